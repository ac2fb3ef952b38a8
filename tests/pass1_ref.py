"""Pass 1 of the intersection, restated in numpy binary32 from its documented rule (tools/gen_pass1.py, trace() in csrc/ssx_kernels.hip) --
not from the generated header's text: the ray set-up, the shear of every quad corner, the five edge functions of a quad, the mixed-sign flag of
its two triangles and, for the plane topology, the behind-the-origin flag.  Returns per ray which triangles are candidates under the generic
rule and under the plane rule, and the figures the CPU proofs count (tests/test_trace_topology_cpu.py).  TEST INFRASTRUCTURE.

The rules:
  set-up   kz = the axis of the direction's largest magnitude, the reference's comparisons (x only if |x| > |y| and |x| > |z|; else y only if
           |y| > |z|; else z: a tie, or a NaN, falls through to the later axis).  (kx, ky) = the other two axes in ascending order.  Sx = d[kx] / d[kz],
           Sy = d[ky] / d[kz], Sz = 1 / d[kz], IEEE binary32 divisions.
  shear    z = v[kz] - o[kz], x = (v[kx] - o[kx]) - Sx * z, y = (v[ky] - o[ky]) - Sy * z: one rounding per operation.
  edges    E(p, q) = p.y * q.x - p.x * q.y.  tri0 = (a, b, c): U = E(b, c), V = E(c, a), W = E(a, b); tri1 = (a, c, d): U = E(c, d), V = E(d, a),
           W = E(a, c) = -V of tri0.
  mixed    a triangle is no candidate iff min3(U, V, W) < 0 < max3(U, V, W) strictly, the minimum and maximum dropping NaN operands.
  behind   (plane rule) a triangle is no candidate either iff its three scaled depths Sz * z are all negative or -0, NaN operands dropped; if all
           three are NaN the flag is the sign of a NaN, which nothing defines: `undetermined`.
"""
import numpy as np

F = np.float32
PERM_AXES = ((1, 2), (0, 2), (0, 1))   # (kx, ky) per kz


def ray_setup(O, D):
    """O, D: [n, 3] float32 -> dict(kz [n], okx, oky, okz, Sx, Sy, Sz [n] float32, tie [n] bool)"""
    O, D = np.asarray(O, dtype=F), np.asarray(D, dtype=F)
    ax, ay, az = (np.abs(D[:, k]) for k in range(3))
    xy = ax > ay
    k0 = xy & (ax > az)
    k1 = ~xy & (ay > az)
    kz = np.where(k0, 0, np.where(k1, 1, 2))
    kx = np.array([p[0] for p in PERM_AXES])[kz]
    ky = np.array([p[1] for p in PERM_AXES])[kz]
    r = np.arange(len(D))
    with np.errstate(all="ignore"):
        dkz = D[r, kz]
        s = dict(kz=kz, kx=kx, ky=ky, okx=O[r, kx], oky=O[r, ky], okz=O[r, kz], Sx=D[r, kx] / dkz, Sy=D[r, ky] / dkz, Sz=F(1.0) / dkz)
    big = np.fmax(np.fmax(ax, ay), az)
    s["tie"] = ((ax == big).astype(int) + (ay == big) + (az == big)) >= 2      # the largest magnitude is reached by two or three components
    return s


def candidates(quads, O, D, ignore=None):
    """quads: [nq][4][3] positions; O, D: [n, 3]; ignore: [n] int or None.
    Returns dict: generic [n, 2 nq] bool (candidate under the generic rule, triangle 2 q + which), plane [n, 2 nq] (generic and not behind),
    culled [n, 2 nq] (generic candidates the behind flag removes), undetermined [n, 2 nq] (all three scaled depths NaN), depth [n, nq, 4] (the scaled
    depths Sz * z of the corners), tie [n], behind_quad [n, nq] (both triangles' depths all negative), straddle [n, nq] (raw depths z of both signs)."""
    V = np.asarray(quads, dtype=F)                               # [nq, 4, 3]
    s = ray_setup(O, D)
    n, nq, r = len(s["kz"]), len(V), np.arange(len(s["kz"]))
    with np.errstate(all="ignore"):
        vx = V[:, :, s["kx"]].transpose(2, 0, 1)                  # [n, nq, 4]
        vy = V[:, :, s["ky"]].transpose(2, 0, 1)
        vz = V[:, :, s["kz"]].transpose(2, 0, 1)
        e = lambda a: a[:, None, None]
        z = vz - e(s["okz"])
        x = (vx - e(s["okx"])) - e(s["Sx"]) * z
        y = (vy - e(s["oky"])) - e(s["Sy"]) * z
        depth = e(s["Sz"]) * z
        E = lambda p, q: y[:, :, p] * x[:, :, q] - x[:, :, p] * y[:, :, q]
        a, b, c, d = 0, 1, 2, 3
        V0 = E(c, a)
        tri = [(E(b, c), V0, E(a, b)), (E(c, d), E(d, a), -V0)]
        corners = [(a, b, c), (a, c, d)]
        generic = np.zeros((n, 2 * nq), dtype=bool); culled = np.zeros_like(generic); undet = np.zeros_like(generic)
        for which in range(2):
            U, Vv, W = tri[which]
            mn, mx = np.fmin(np.fmin(U, Vv), W), np.fmax(np.fmax(U, Vv), W)
            mixed = (mn < 0) & (mx > 0)
            dz = depth[:, :, list(corners[which])]                # [n, nq, 3]
            nan = np.isnan(dz)
            behind = (nan | np.signbit(dz)).all(axis=2) & ~nan.all(axis=2)
            generic[:, which::2] = ~mixed
            culled[:, which::2] = ~mixed & behind
            undet[:, which::2] = nan.all(axis=2)
    if ignore is not None:
        ign = np.asarray(ignore).astype(np.int64)
        ok = (ign >= 0) & (ign < nq)
        for which in range(2):
            generic[r[ok], 2 * ign[ok] + which] = False
            culled[r[ok], 2 * ign[ok] + which] = False
    with np.errstate(all="ignore"):
        behind_quad = (np.signbit(depth) & ~np.isnan(depth)).all(axis=2)
        straddle = (z < 0).any(axis=2) & (z > 0).any(axis=2)
    return dict(generic=generic, plane=generic & ~culled, culled=culled, undetermined=undet, depth=depth, tie=s["tie"], behind_quad=behind_quad,
                straddle=straddle, kz=s["kz"])
