"""Crafted scenes that force the rare branches of the integrator (reference file:line in each
builder), for both sides of the parity tests.  TEST INFRASTRUCTURE (uses tests/custom_scene.py)."""
import numpy as np

import custom_scene as cs

# materials of the base scene "cornell" (oracle_scene.c / src/scene.cpp:66-110)
WHITE, GREEN, RED, LIGHT = 0, 3, 4, 5


def _room(c, lo=-4.0, hi=4.0, mat=WHITE):
    """closed axis-aligned box, normals inward (vertex order as the reference's plane-srgb box, src/scene.cpp:372-409)"""
    l, h = lo, hi
    c.add_quad((l, l, h), (l, l, l), (l, h, l), (l, h, h), mat)
    c.add_quad((h, l, l), (h, l, h), (h, h, h), (h, h, l), GREEN)
    c.add_quad((l, l, h), (h, l, h), (h, l, l), (l, l, l), mat)
    c.add_quad((h, h, h), (l, h, h), (l, h, l), (h, h, l), mat)
    c.add_quad((l, l, l), (h, l, l), (h, h, l), (l, h, l), RED)
    c.add_quad((h, l, h), (l, l, h), (l, h, h), (h, h, h), mat)


def degenerate_light_scene(view="edge_ab"):
    """SphericalTriangle's degenerate ladder (src/util/spherical-tri.cpp:74-123), zero-area light
    triangles (pdf = 1/0, src/geometry.cpp:115) and a light too small to subtend an angle.

    A unit light quad hangs at y = 1.  Small receiver quads sit ON THE EXTENSION of two of its
    edges, so that from every point of them two of the three directions toward a light triangle's
    vertices coincide (their dot product rounds to 1.0f, the side is 0, its sine is 0):
      view "edge_ab": receiver beyond v10 on the line v00-v10 -> side c of tri0 is 0 (:85-92: alpha = pi/2)
      view "edge_bc": receiver beyond v11 on the line v10-v11 -> side a of tri0 is 0 (:105-113: alpha = acos(.))
      view "far":     a second, 1e-4-sized light seen from metres away -> all sides 0 (:114-122: NaN)
      view "room":    the whole room (every branch mixed with regular paths)
    The second light's tri0 is collapsed (v10 == v11): zero area, NaN normal, can never be hit, but is
    sampled with probability 1/4."""
    c = cs.CustomScene("cornell", keep_quads=False)
    _room(c)
    c.add_quad((0, 1, 0), (1, 1, 0), (1, 1, 1), (0, 1, 1), LIGHT)                      # quad 6: the light, facing down
    e = 2e-3
    c.add_quad((3, 1 - e, -e), (3, 1 - e, e), (3, 1 + e, e), (3, 1 + e, -e), WHITE)    # 7: on the line through v00-v10 (x axis at y=1, z=0)
    c.add_quad((1 - e, 1 - e, 3), (1 + e, 1 - e, 3), (1 + e, 1 + e, 3), (1 - e, 1 + e, 3), WHITE)  # 8: on the line through v10-v11
    t = 1e-4
    c.add_quad((-2, 2, -2), (-2 + t, 2, -2), (-2 + t, 2, -2), (-2, 2, -2 + t), LIGHT)  # 9: tiny light, tri0 collapsed
    if view == "edge_ab":
        c.set_camera((2.0, 1.0, 0.0), (3.0, 1.0, 0.0), up=(0, 1, 0), vfov_deg=0.2)
    elif view == "edge_bc":
        c.set_camera((1.0, 1.0, 2.0), (1.0, 1.0, 3.0), up=(0, 1, 0), vfov_deg=0.2)
    elif view == "far":
        c.set_camera((3.0, -3.0, 3.0), (3.9, -3.9, 3.9), up=(0, 1, 0), vfov_deg=30.0)
    else:
        c.set_camera((3.5, -3.0, -3.5), (0.0, 0.5, 0.5), up=(0, 1, 0), vfov_deg=60.0)
    return c


def shared_edge_scene():
    """Rays through shared vertices and edges: the f64 fallback of the watertight test
    (src/geometry.cpp:56-67) and its tie rules (strict '<', first quad in list order wins,
    src/scene.cpp:433-445; tri0 before tri1, src/geometry.cpp:128-139).  Four coplanar quads meet in
    one vertex on the camera axis; the field of view is a few float ulps wide, so most camera rays
    have an edge function that is exactly 0 in float."""
    c = cs.CustomScene("cornell", keep_quads=False)
    _room(c)
    c.add_quad((-1, 3.9, -1), (1, 3.9, -1), (1, 3.9, 1), (-1, 3.9, 1), LIGHT)
    z = 1.0
    c.add_quad((0, 0, z), (1, 0, z), (1, 1, z), (0, 1, z), WHITE)
    c.add_quad((-1, 0, z), (0, 0, z), (0, 1, z), (-1, 1, z), GREEN)
    c.add_quad((-1, -1, z), (0, -1, z), (0, 0, z), (-1, 0, z), RED)
    c.add_quad((0, -1, z), (1, -1, z), (1, 0, z), (0, 0, z), WHITE)
    c.set_camera((0.0, 0.0, -2.0), (0.0, 0.0, 1.0), up=(0, 1, 0), vfov_deg=2e-5)
    return c


def triangle_scene():
    """Top-level PrimTri primitives (src/geometry.hpp:55-74, src/scene.hpp:39-41): one as a LIGHT -- sampled by
    PrimTri::get_rand_toward (src/geometry.cpp:103-116): no triangle pick, so one random number fewer than a quad
    light, and no halving of the pdf (:141-145) -- next to a quad light (the light pick, src/scene.cpp:417-431,
    then mixes both kinds), two as occluders (one triangle each: where a quad's second triangle would be, rays pass)."""
    c = cs.CustomScene("cornell", keep_quads=False)
    _room(c)
    c.add_tri((-3, 3.9, -3), (-1, 3.9, -3), (-3, 3.9, -1), LIGHT)                    # 6: triangle light under the ceiling
    c.add_quad((1, 3.9, 1), (2.5, 3.9, 1), (2.5, 3.9, 2.5), (1, 3.9, 2.5), LIGHT)    # 7: quad light
    c.add_tri((-2.5, 0.5, 0.5), (0.5, 0.5, 0.0), (-1.0, 0.5, 2.5), GREEN)             # 8: a triangle hovering over the floor
    c.add_tri((0.0, -1.0, -1.0), (2.0, -1.5, 0.0), (1.0, 1.5, 0.5), RED)              # 9: a tilted one
    c.add_quad((-3.5, -4 + 1e-3, -3.5), (-1.5, -4 + 1e-3, -3.5), (-1.5, -4 + 1e-3, -1.5), (-3.5, -4 + 1e-3, -1.5), WHITE)  # 10: a quad after the triangles
    c.set_camera((3.4, -2.5, -3.4), (-0.5, 0.3, 0.5), up=(0, 1, 0), vfov_deg=65.0)
    return c


def many_prims_scene(n_prims, observer=1931, seed=9):
    """More than 32 primitives (the reference's Scene::intersect loops over any number, src/scene.cpp:433-445): the room, then
    a cloud of small quads and triangles in all orientations, lights among them at list positions in different groups of
    32, the last primitive a light too.  n_prims = 70 with the CIE 1931 tables keeps every table in LDS; 128 with the
    CIE 2006 tables overflows it: the permuted vertex table is then read from HBM."""
    g = np.random.default_rng(seed)
    c = cs.CustomScene("cornell", observer=observer, keep_quads=False)
    _room(c)
    mats = (WHITE, GREEN, RED)
    light_at = {6, 20, 33, 64, 97, n_prims - 1}
    while len(c.quads) < n_prims:
        i = len(c.quads)
        ctr = g.uniform(-3.2, 3.2, size=3)
        u = g.normal(size=3); u /= np.linalg.norm(u)
        v = np.cross(u, g.normal(size=3)); v /= np.linalg.norm(v)
        su, sv = g.uniform(0.25, 0.9, size=2)
        m = LIGHT if i in light_at else mats[i % 3]
        p00, p10, p11, p01 = ctr - su * u - sv * v, ctr + su * u - sv * v, ctr + su * u + sv * v, ctr - su * u + sv * v
        if i % 5 == 3:
            c.add_tri(p00, p10, p11, m)
        else:
            c.add_quad(p00, p10, p11, p01, m)
    c.set_camera((3.6, 0.2, -3.6), (0.0, 0.0, 0.0), up=(0, 1, 0), vfov_deg=70.0)
    return c


def many_textures_scene(n_textures=9, seed=4):
    """The Cornell box with every wall, the floor and the faces of the short block on textures of their own (different sizes,
    incl. 1 x 1 and non-square): more textures than the reference's scenes use (src/scene.cpp: one); MaterialLambertian holds
    any texture per material (src/material.cpp:10-29)."""
    g = np.random.default_rng(seed)
    c = cs.CustomScene("cornell-srgb")
    sizes = [(1, 1), (2, 3), (7, 5), (16, 16), (33, 9), (64, 48), (5, 128), (31, 31), (256, 2), (12, 12), (3, 3), (8, 1)]
    targets = [0, 6, 7, 9, 10, 11, 12, 13, 2, 3, 4, 5]
    for k in range(n_textures - len(c.textures)):
        h, w = sizes[k % len(sizes)]
        c.textures.append(g.integers(0, 256, size=(h, w, 3), dtype=np.uint8))
        if k < len(targets): # (textures beyond the quads at hand are uploaded and unused)
            m = c.add_material(albedo_texture=len(c.textures) - 1)
            pos, st, _ = c.quads[targets[k]]
            c.quads[targets[k]] = (pos, st, m)
    return c


def random_scene(seed):
    """A scene drawn from `seed`: 3..40 (one in six: up to 115) quads and triangles of all sizes and orientations, sometimes inside a closed room, with
    Lambertian (constant / textured), mirror and emissive materials, at least one light (quad or triangle), a random camera.
    Returns (scene, render options): indirect_only / explicit light sampling / flat-field correction are drawn as well.  The
    differential fuzz of the parity tests: combinations no hand-made scene has (a mirror next to a triangle light in a build
    without explicit light sampling, textures on triangles, lights seen edge-on, ...)."""
    g = np.random.default_rng(1000 + seed)
    c = cs.CustomScene("cornell-srgb", keep_quads=False, observer=(1931, 2006)[int(g.integers(0, 4) == 0)])
    mats = [WHITE, GREEN, RED]
    white_spectrum = c.materials[WHITE]["albedo_spectrum"]
    mats.append(c.add_material(kind=1, albedo_spectrum=white_spectrum))                 # a mirror (src/material.cpp:146-167)
    for _ in range(int(g.integers(0, 3))):                                              # up to two more textures
        h, w = (int(v) for v in g.integers(1, 24, size=2))
        c.textures.append(g.integers(0, 256, size=(h, w, 3), dtype=np.uint8))
    for t in range(len(c.textures)):
        mats.append(c.add_material(albedo_texture=t))
    if g.integers(0, 2):
        _room(c, mat=mats[int(g.integers(0, len(mats)))])
    n = int(g.integers(3, 41)) if g.integers(0, 6) else int(g.integers(41, 110))      # one scene in six: several groups of 32 primitives
    n_lights = 0
    while len(c.quads) < n or n_lights == 0:
        ctr = g.uniform(-3.0, 3.0, size=3)
        u = g.normal(size=3); u /= np.linalg.norm(u)
        v = np.cross(u, g.normal(size=3)); v /= np.linalg.norm(v)
        su, sv = np.exp(g.uniform(np.log(0.05), np.log(2.5), size=2))
        light = g.integers(0, 6) == 0 or (len(c.quads) >= n and n_lights == 0)
        m = LIGHT if light else mats[int(g.integers(0, len(mats)))]
        n_lights += int(light)
        skew = g.uniform(-0.3, 0.3) * su * u if g.integers(0, 3) == 0 else 0.0 * u       # some quads are not rectangles
        p00, p10, p11, p01 = ctr - su * u - sv * v, ctr + su * u - sv * v, ctr + su * u + sv * v + skew, ctr - su * u + sv * v
        if g.integers(0, 4) == 0:
            c.add_tri(p00, p10, p11, m)
        else:
            c.add_quad(p00, p10, p11, p01, m)
    eye = g.uniform(-3.8, 3.8, size=3)
    c.set_camera(tuple(eye), tuple(g.uniform(-1.0, 1.0, size=3)), up=(0, 1, 0), vfov_deg=float(g.uniform(20.0, 90.0)))
    opts = dict(indirect_only=bool(g.integers(0, 4) == 0), els=bool(g.integers(0, 3) != 0), flat_field=bool(g.integers(0, 4) != 0))
    return c, opts


def origin_light_scene():
    """A light with a vertex exactly at the origin: shading points a denormal-ish distance from it give squared lengths below
    2^-100, outside the proven domain of the kernel's fast exact sqrt (csrc/ssx_exact.h) -- the kernel must take the plain IEEE
    path there (normalize3_any, func_bar) and still equal the reference's glm::normalize."""
    c = cs.CustomScene("cornell", keep_quads=False)
    _room(c)
    c.add_quad((0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1), LIGHT)
    c.set_camera((2.0, 2.0, -3.0), (0.5, 0.0, 0.5), up=(0, 1, 0), vfov_deg=40.0)
    return c


def _distinct_corners(c):
    """{position bits: position} over the corners of the scene's quads, in order of first occurrence"""
    pts = {}
    for pos, _, _ in c.quads:
        for p in pos:
            pts.setdefault(np.asarray(p, dtype=np.float32).tobytes(), np.asarray(p, dtype=np.float64))
    return pts


def warped_builtin(seed):
    """One of the reference's built-in scenes (src/scene.cpp:32-415) with every distinct corner moved -- the same way wherever it occurs, so the
    corners still coincide in the built-in pattern and the library keeps the kernel whose pass 1 is specialised to that mesh topology
    (csrc/ssx_pass1_gen.h: the sharing pattern is compiled in, positions are run-time data).  The random scenes of `random_scene` run the generic
    kernel or one compiled at upload; this is the fuzz of the kernels the headline numbers are measured on: the Cornell box and the plane scene
    rotated, scaled by 2^-10 .. 2^10 and translated (the light stays in the ceiling's plane: shadow rays inside the plane of ten triangles, now
    along no axis), with every corner jittered (quads that are neither planar nor rectangles, lights included, rooms that leak), flattened into
    slivers, or sheared -- with a camera that follows.  Returns (scene, name of the base scene, render options)."""
    g = np.random.default_rng(5000 + seed)
    base = ("cornell-srgb", "plane-srgb", "cornell")[seed % 3]
    kind = (seed // 3) % 4            # 0: similarity, 1: jitter, 2: similarity + jitter, 3: flatten + shear
    c = cs.CustomScene(base, observer=(1931, 2006)[int(g.integers(0, 4) == 0)])
    pts = _distinct_corners(c)
    allp = np.array(list(pts.values()))
    ctr = 0.5 * (allp.min(axis=0) + allp.max(axis=0))
    size = float(np.abs(allp - ctr).max())
    q, _ = np.linalg.qr(g.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    if kind in (0, 2):
        s = 2.0 ** float(g.integers(-10, 11))
        A = s * q
        new_ctr = ctr * s + g.uniform(-1.0, 1.0, size=3) * size * s
    elif kind == 3:
        flat = np.diag([1.0, 1.0, 2.0 ** float(-g.integers(3, 13))])           # one axis of a rotated frame pressed flat: every triangle a sliver from most directions
        shear = np.eye(3); shear[0, 1] = g.uniform(-0.8, 0.8)
        A = q @ flat @ shear @ q.T
        new_ctr = ctr
    else:
        A = np.eye(3)
        new_ctr = ctr
    amp = 0.03 * size if kind in (1, 2) else 0.0
    while True:
        moved = {k: (A @ ((p + g.normal(size=3) * amp) - ctr) + new_ctr).astype(np.float32) for k, p in pts.items()}
        if len({m.tobytes() for m in moved.values()}) == len(moved):               # distinct corners stay distinct (else the sharing pattern would change)
            break
    for i, (pos, st, m) in enumerate(c.quads):
        c.quads[i] = (np.array([moved[np.asarray(p, dtype=np.float32).tobytes()] for p in pos], dtype=np.float32), st, m)
    eye = A @ (c.cam_pos.astype(np.float64) - ctr) + new_ctr
    target = new_ctr + A @ (g.uniform(-0.2, 0.2, size=3) * size)
    if kind == 3 and base != "plane-srgb":                                         # (the flattened box seen from its opening is a line: look around from inside)
        eye = new_ctr + A @ (g.uniform(-0.35, 0.35, size=3) * size)
        target = new_ctr + A @ (g.uniform(-0.35, 0.35, size=3) * size)
    up = A @ np.array([0.0, 1.0, 0.0]); up /= np.linalg.norm(up)
    c.set_camera(tuple(eye), tuple(target), up=tuple(up), vfov_deg=float(g.uniform(30.0, 70.0)))
    opts = dict(indirect_only=bool(g.integers(0, 4) == 0), els=bool(g.integers(0, 4) != 0), flat_field=bool(g.integers(0, 4) != 0))
    return c, base, opts


def islands_scene(seed=21):
    """32 quads that share no corner at all: 128 distinct vertices, the most a topology-specialised trace can meet (both flag accumulators of pass 1
    full, the largest offsets of the distinct-vertex table).  A room whose six sides are each tiled by four overlapping quads in front of a fifth
    that backs them -- every corner jittered, so no two coincide and no quad is planar or a rectangle -- with a light under the ceiling and a
    tilted quad in the middle.  Rays from inside hit something almost always; most meet two or three candidates per side."""
    g = np.random.default_rng(seed)
    c = cs.CustomScene("cornell", keep_quads=False)
    mats = (WHITE, GREEN, RED)
    R = 4.0
    frames = []   # (outward axis, sign): the side's plane is x[axis] = sign * R, its quads wind like _room's (normals inward is not required here)
    for axis in range(3):
        for sign in (-1.0, 1.0):
            frames.append((axis, sign))
    jit = lambda p: tuple(np.asarray(p, dtype=np.float64) + g.uniform(-0.08, 0.08, size=3))
    for axis, sign in frames:
        u, v = [k for k in range(3) if k != axis]
        def corner(s, t, depth):
            p = np.zeros(3); p[axis] = sign * (R + depth); p[u] = s; p[v] = t
            return jit(p)
        for i, (s0, t0) in enumerate(((-R, -R), (-0.3, -R), (-R, -0.3), (-0.3, -0.3))):       # four tiles of 4.3 x 4.3: they overlap by 0.6 in the middle
            s1, t1 = s0 + R + 0.3, t0 + R + 0.3
            c.add_quad(corner(s0, t0, 0.0), corner(s1, t0, 0.0), corner(s1, t1, 0.0), corner(s0, t1, 0.0), mats[(i + axis) % 3])
        c.add_quad(corner(-R - 0.5, -R - 0.5, 0.4), corner(R + 0.5, -R - 0.5, 0.4), corner(R + 0.5, R + 0.5, 0.4), corner(-R - 0.5, R + 0.5, 0.4), WHITE)
    c.add_quad(jit((-1, 3.5, -1)), jit((1, 3.5, -1)), jit((1, 3.5, 1)), jit((-1, 3.5, 1)), LIGHT)
    c.add_quad(jit((-1.5, -1.0, -0.5)), jit((1.0, -1.5, 0.5)), jit((1.5, 1.0, 1.0)), jit((-1.0, 1.5, -1.0)), GREEN)
    assert len(c.quads) == 32 and len(_distinct_corners(c)) == 128
    c.set_camera((3.0, 0.5, -3.0), (0.0, 0.0, 0.0), up=(0, 1, 0), vfov_deg=60.0)
    return c


def fan_scene():
    """One vertex that belongs to eight quads, and quads that share two edges: a cone of eight quads around its apex -- each shares an edge with
    both neighbours, and the apex takes every one of the four corner slots in turn, so the shared edges are diagonals, first and last edges -- inside
    a closed room (eight corners shared three ways), under a light, next to a pair of quads that share two edges WITH EACH OTHER (v00-v10 and v10-v11)."""
    c = cs.CustomScene("cornell", keep_quads=False)
    _room(c)
    c.add_quad((-1, 3.9, -1), (1, 3.9, -1), (1, 3.9, 1), (-1, 3.9, 1), LIGHT)
    apex = (0.25, 1.0, -0.5)
    ang = [2.0 * np.pi * k / 8 + 0.1 for k in range(8)]
    ring = [(0.25 + 1.5 * np.cos(t), -0.5, -0.5 + 1.5 * np.sin(t)) for t in ang]
    outer = [(0.25 + 3.0 * np.cos(t + np.pi / 8), -2.0, -0.5 + 3.0 * np.sin(t + np.pi / 8)) for t in ang]
    mats = (WHITE, GREEN, RED)
    for k in range(8):
        four = [apex, ring[k], outer[k], ring[(k + 1) % 8]]
        four = four[-(k % 4):] + four[:-(k % 4)] if k % 4 else four             # the apex as v00, v10, v11, v01 in turn
        c.add_quad(*four, mats[k % 3])
    A, B, Cc = (-3.0, -3.0, 2.0), (-1.0, -3.5, 2.5), (-1.0, -1.0, 3.0)
    c.add_quad(A, B, Cc, (-3.0, -1.0, 2.0), RED)
    c.add_quad(A, B, Cc, (-3.5, -0.5, 3.5), GREEN)
    n_apex = sum(1 for pos, _, _ in c.quads if any(np.asarray(p, dtype=np.float32).tobytes() == np.asarray(apex, dtype=np.float32).tobytes() for p in pos))
    assert n_apex == 8 and len(c.quads) == 17
    c.set_camera((3.4, 2.5, -3.4), (0.0, -0.5, 0.0), up=(0, 1, 0), vfov_deg=65.0)
    return c


# ---- the scenes of tests/test_trace_topology_{cpu,gpu}.py: (name, topology the context must report) ------------------------------------------------------
TRACE_TOPO_SCENES = (("cornell-srgb", 1), ("cornell", 1), ("warped-cornell-a", 1), ("warped-cornell-b", 1),
                     ("plane-srgb", 2), ("warped-plane-a", 2), ("warped-plane-b", 2),
                     ("moved-corner", 3), ("islands32", 3), ("fan", 3))
# seeds of warped_builtin: seed % 3 picks the base scene (0 cornell-srgb, 1 plane-srgb, 2 cornell), (seed // 3) % 4 the kind of warp
_TRACE_TOPO_WARPS = {"warped-cornell-a": 6, "warped-cornell-b": 11, "warped-plane-a": 7, "warped-plane-b": 22}


def trace_topo_scene(name):
    """(CustomScene, renderer options) of one entry of TRACE_TOPO_SCENES; one object per process (matrix_case's rule)."""
    key = ("trace-topo", name)
    if key in _matrix_cache:
        return _matrix_cache[key]
    T = MATRIX_TEX
    if name in ("cornell-srgb", "cornell", "plane-srgb"):
        c, base = cs.CustomScene(name), name
    elif name in _TRACE_TOPO_WARPS:
        c, base, _ = warped_builtin(_TRACE_TOPO_WARPS[name])
    elif name == "moved-corner":
        c, base = matrix_case("moved-corner").scene, "cornell-srgb"
    elif name == "islands32":
        c, base = islands_scene(), "cornell"
    elif name == "fan":
        c, base = fan_scene(), "cornell"
    else:
        raise KeyError(name)
    topo = dict(TRACE_TOPO_SCENES)[name]
    opts = dict(scene_name=base, observer=c.observer, texture=None if base == "cornell" else T, res=(8, 8), spp=1, jit_pass1=topo == 3)
    _matrix_cache[key] = (c, opts)
    return c, opts


# ---- the scene and option matrix of tests/test_pipeline_matrix_{cpu,gpu}.py -------------------------------------------------------------------------------
# Every scene and switch the path kernel is tested on, as (oracle, renderer) pairs for the kernels behind it: the _flux twins, the bin kernel, the guides,
# the noise estimate, the filter chain and the develop.

MATRIX_TEX = "test-img.png"
# "fuzz" has triangles, so it runs the generic kernel; "warped" keeps the mesh topology of its built-in scene and with it the built-in topology kernel, whatever
# ssx_set_jit says; "moved-corner" matches no built-in topology and is the case with its run-time compiled kernels (jit_pass1=True: the plain ones at upload,
# their _flux twins at the first render with spectral output on).  "plane-indirect" is black (MATRIX_BLACK); "cornell-indirect" is the indirect_only case in
# which light does arrive.
MATRIX_CASES = ("triangles", "prims70", "prims128-2006", "textures", "shared-edge", "fuzz", "warped", "moved-corner", "mirror", "observer2006", "jh", "meng",
                "cornell-no-els", "prims70-no-els", "plane-indirect", "cornell-indirect", "cornell-no-ffc")
JIT_PASS1 = "scene topology (compiled at upload)"
FUZZ_SEED, WARPED_SEED = 7, 3
MATRIX_BLACK = ("plane-indirect",)    # every camera ray hits, no flux arrives: the bins hold counts and sums of 0 (and one primitive fills the view)


class MatrixCase:
    """One case: `oracle` (ol.Oracle, with the case's observer, uplift and materials), `flags` (indirect_only / els / flat_field for Oracle.render and
    Oracle.samples), `pass1` (the kernel variant plan_info() must name), `scene` (the CustomScene, or None for a built-in one) and `renderer(res)`."""

    def __init__(self, name, oracle, options, flags=None, scene=None, pass1="generic", mirror_quads=None):
        self.name, self.oracle, self.options, self.scene, self.pass1, self.mirror_quads = name, oracle, options, scene, pass1, mirror_quads
        self.jit = pass1 == JIT_PASS1
        self.flags = dict(indirect_only=False, els=True, flat_field=True)
        self.flags.update(flags or {})
        self._keep = []

    def renderer(self, res, seed=5, **opts):
        import ctypes as C
        from simple_spectral_amd import Options, Renderer, _capi
        o = dict(res=res, seed=seed, jit_pass1=self.jit, indirect_only=self.flags["indirect_only"], explicit_light_sampling=self.flags["els"],
                 flat_field_correction=self.flags["flat_field"])
        o.update(self.options); o.update(opts)
        r = Renderer(Options(**o))
        if self.scene is not None:
            r.upload_scene_desc(self.scene.desc(self.oracle))
        if self.mirror_quads is not None:                                # as tests/test_gpu_parity.py test_mirror_material_bit_exact switches them
            d = r.scene.desc.contents
            mats = (_capi.SsxMaterial * d.n_materials)(*[d.materials[i] for i in range(d.n_materials)])
            for q in range(d.n_quads):
                if self.mirror_quads(q):
                    mats[d.quads[q].material].kind = 1                    # SSX_MTL_MIRROR
            d2 = _capi.SsxSceneDesc.from_buffer_copy(d)
            d2.materials = C.cast(mats, C.POINTER(_capi.SsxMaterial))
            self._keep.append(mats)
            r._check(r._lib.ssx_upload_scene(r._ctx, C.byref(d2)))
        return r

    def render_ref(self, W, H, spp, seed=5):
        return self.oracle.render(W, H, spp, seed=seed, **self.flags)

    def samples_ref(self, W, H, spp, seed=5):
        return self.oracle.samples(W, H, spp, seed=seed, **self.flags)

    def light_prims(self):
        import ctypes as C
        nl = C.c_int()
        self.oracle.lib.orc_scene_counts(self.oracle.scene, None, C.byref(nl), None)
        return {int(self.oracle.lib.orc_scene_light(self.oracle.scene, i)) for i in range(nl.value)}


_matrix_cache = {}


def _meng_grid():
    """(table, path of the grid file the host library reads): the table of tests/golden/ref_vectors.npz, written once per process"""
    if "meng" not in _matrix_cache:
        import atexit, os, tempfile
        import ref_lib
        from simple_spectral_amd import meng
        table = ref_lib.meng_table()
        fd, path = tempfile.mkstemp(suffix=".bin", prefix="ssx-meng-grid-")
        os.close(fd)
        meng.save_table(path, table)
        atexit.register(lambda: os.path.exists(path) and os.remove(path))
        _matrix_cache["meng"] = (table, path)
    return _matrix_cache["meng"]


def matrix_case(name):
    """The case `name` of MATRIX_CASES; one object per process (a CustomScene's description points into the scene's own arrays)."""
    if name in _matrix_cache:
        return _matrix_cache[name]
    import oracle_lib as ol
    from simple_spectral_amd.renderer import Scene
    T = MATRIX_TEX
    custom = lambda c, **kw: MatrixCase(name, c.oracle(), dict(scene_name="cornell", observer=c.observer), scene=c, **kw)
    builtin = lambda scene, oracle, pass1, flags=None, mirror_quads=None, **o: MatrixCase(name, oracle, dict(scene_name=scene, texture=T, **o), flags=flags,
                                                                                         pass1=pass1, mirror_quads=mirror_quads)
    if name == "triangles":
        case = custom(triangle_scene())
    elif name == "prims70":
        case = custom(many_prims_scene(70, 1931))
    elif name == "prims128-2006":
        case = custom(many_prims_scene(128, 2006))
    elif name == "textures":
        case = custom(many_textures_scene(), pass1="cornell topology")      # (materials and textures changed, the mesh is the Cornell box's)
    elif name == "shared-edge":
        case = custom(shared_edge_scene())
    elif name == "fuzz":
        c, o = random_scene(FUZZ_SEED)
        case = custom(c, flags=o)
    elif name == "warped":
        c, base, o = warped_builtin(WARPED_SEED)
        case = MatrixCase(name, c.oracle(), dict(scene_name=base, observer=c.observer, texture=None if base == "cornell" else T), flags=o, scene=c,
                          pass1="plane topology" if base == "plane-srgb" else "cornell topology")
    elif name == "moved-corner":
        # The Cornell box with one corner moved apart from its twins: a corner that no other test module moves (the compiled code of a sharing pattern stays
        # in the process's memory, and the modules that upload their own moved-corner boxes expect the generic kernel for them when they run first).
        c = cs.CustomScene("cornell-srgb")
        pos, st, m = c.quads[3]
        pos = pos.copy(); pos[2, 1] += 0.5
        c.quads[3] = (pos, st, m)
        case = MatrixCase(name, c.oracle(), dict(scene_name="cornell-srgb", texture=T), scene=c, pass1=JIT_PASS1)
    elif name == "cornell-indirect":
        case = builtin("cornell-srgb", ol.Oracle("cornell-srgb", texture=T), "cornell topology", flags=dict(indirect_only=True))
    elif name == "mirror":
        orc = ol.Oracle("cornell-srgb", texture=T)
        pick = lambda q: q >= 9
        nq = ol.C.c_int()
        orc.lib.orc_scene_counts(orc.scene, ol.C.byref(nq), None, None)
        for q in range(nq.value):
            if pick(q):
                assert orc.lib.orc_scene_set_material_kind(orc.scene, orc.lib.orc_scene_quad_material(orc.scene, q), 1) == 0
        case = builtin("cornell-srgb", orc, "cornell topology", mirror_quads=pick)
    elif name == "observer2006":
        case = builtin("cornell-srgb", ol.Oracle("cornell-srgb", observer=2006, texture=T), "cornell topology", observer=2006)
    elif name == "jh":
        model = Scene("cornell-srgb", texture=T, uplift="jh", jh_res=16).jh_model()
        case = builtin("cornell-srgb", ol.Oracle("cornell-srgb", texture=T, jh=model), "cornell topology", uplift="jh", jh_res=16)
    elif name == "meng":
        table, path = _meng_grid()
        case = builtin("cornell-srgb", ol.Oracle("cornell-srgb", texture=T, meng=table), "cornell topology", uplift="meng", meng_grid_path=path)
    elif name == "cornell-no-els":
        case = builtin("cornell-srgb", ol.Oracle("cornell-srgb", texture=T), "cornell topology", flags=dict(els=False))
    elif name == "prims70-no-els":
        case = custom(many_prims_scene(70, 1931), flags=dict(els=False))
    elif name == "plane-indirect":
        case = builtin("plane-srgb", ol.Oracle("plane-srgb", texture=T), "plane topology", flags=dict(indirect_only=True))
    elif name == "cornell-no-ffc":
        case = builtin("cornell-srgb", ol.Oracle("cornell-srgb", texture=T), "cornell topology", flags=dict(flat_field=False))
    else:
        raise KeyError(name)
    _matrix_cache[name] = case
    return case
