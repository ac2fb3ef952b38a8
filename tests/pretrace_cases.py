"""The cases of the camera-ray pre-trace tests (tests/test_pretrace_cpu.py, tests/test_pretrace_gpu.py, tests/pretrace_worker.py): the scenes and
image layouts whose tile masks are read back, the mask families of the masked-trace unit op, and the scenes rendered whole in the mode the
calibration does not choose for them.  TEST INFRASTRUCTURE; everything here is computed on the CPU, once per process."""
import functools

import numpy as np

import crafted
import custom_scene as cs
import tile_mask_ref as tm
import unit_cases as uc


def _inside_looking_at_a_corner():
    """many_prims_scene(70) seen from the room's centre towards a corner: most primitives are behind the camera"""
    c = crafted.many_prims_scene(70)
    c.set_camera((0.0, 0.0, 0.0), (4.0, 4.0, 4.0), up=(0, 1, 0), vfov_deg=70.0)
    return c


# name -> (scene builder, (width, height), tile_first / tile_stride / tile_skew of the render)
MASK_CASES = {
    "cornell-srgb": (lambda: cs.CustomScene("cornell-srgb"), (24, 16), {}),
    "prims33": (lambda: crafted.many_prims_scene(33), (32, 24), {}),
    "prims70": (lambda: crafted.many_prims_scene(70), (32, 24), {}),
    "prims128-2006": (lambda: crafted.many_prims_scene(128, 2006), (32, 24), {}),          # permuted table in HBM; the g == 1 half of the mask kernel
    "triangles": (crafted.triangle_scene, (24, 24), {}),
    "prims70-ragged": (lambda: crafted.many_prims_scene(70), (27, 21), dict(tile_first=1, tile_stride=3)),
    "prims70-inside": (_inside_looking_at_a_corner, (32, 24), {}),
}
# the scenes of the masked-trace op: the geometry of the cases above (a camera or an image layout does not enter a trace)
TRACE_SCENES = ("cornell-srgb", "prims33", "prims70", "prims128-2006", "triangles")


@functools.lru_cache(maxsize=None)
def mask_case(name):
    """(scene, oracle, (W, H), layout dict with tile_first / tile_stride / tile_skew) -- one object per process"""
    build, res, layout = MASK_CASES[name]
    c = build()
    full = dict(tile_first=0, tile_stride=1, tile_skew=0)
    full.update(layout)
    return c, c.oracle(), res, full


@functools.lru_cache(maxsize=None)
def reference(name):
    """(tile_mask_ref.Mask by the documented rule, [(tx, ty)] per slot, the scene description's arrays)"""
    c, orc, (W, H), lay = mask_case(name)
    arrays = tm.scene_arrays(c.desc(orc))
    return tm.reference_mask(*arrays, W, H, **lay), tm.slot_tiles(W, H, **lay), arrays


@functools.lru_cache(maxsize=None)
def ground_truth(name):
    """bool [slots, n_prims]: the primitives the tile's rays hit, by the oracle's intersection (tile_mask_ref.tiles_hit)"""
    c, orc, (W, H), lay = mask_case(name)
    _, tiles, (pv_inv, cam_pos, _) = reference(name)
    return tm.tiles_hit(orc, pv_inv, cam_pos, W, H, tiles)


# ---- the masked trace: rows, the oracle's results, mask families ---------------------------------------------------------------------------
MISS = 0xFFFFFFFF
WATCHED_Q = (15, 16, 17, 31)    # places of a group of 32 around the seam of the two flag accumulators, and the last one


@functools.lru_cache(maxsize=None)
def trace_rows(name):
    """(rows uint32 [n, 7] of SSX_DBG_TRACE, the oracle's result [n, 5], number of primitives)"""
    c, orc, _, _ = mask_case(name)
    w = uc.trace_inputs([q[0] for q in c.quads], n_random=1500)
    ref, _ = uc.oracle_trace(orc, w)
    ref.setflags(write=False); w.setflags(write=False)
    return w, ref, len(c.quads)


def words_of(bits):
    """bool [n_prims] -> the four mask words"""
    return tm.pack(np.asarray(bits, dtype=bool)[None, :])[0]


class Blocks:
    """Rows laid out for SSX_DBG_TRACE_MASKED: `index` [64 * blocks] into the case's rows (a short block is padded with its final row), `masks`
    uint32 [blocks, 4]; `rows()` = the op's input [64 * blocks, 11]."""

    def __init__(self, name, groups, masks):
        self.name = name
        self.index = np.concatenate([np.concatenate([g, np.full(64 - len(g), g[-1])]) for g in groups]).astype(np.int64)
        self.masks = np.asarray(masks, dtype=np.uint32).reshape(len(groups), 4)
        assert all(0 < len(g) <= 64 for g in groups)

    def rows(self):
        w, _, _ = trace_rows(self.name)
        return np.ascontiguousarray(np.concatenate([w[self.index], np.repeat(self.masks, 64, axis=0)], axis=1))

    def expected(self):
        return trace_rows(self.name)[1][self.index]

    def kept(self):
        """bool [64 * blocks, n_prims]: the row's mask, per primitive"""
        return np.repeat(tm.unpack(self.masks, trace_rows(self.name)[2]), 64, axis=0)


def _chunks(idx):
    return [idx[i:i + 64] for i in range(0, len(idx), 64)]


def _random_bits(g, n):
    """n mask bits, group of 32 by group: nothing, a few, about half, or all of them"""
    bits = np.zeros(n, dtype=bool)
    for base in range(0, n, 32):
        m = min(32, n - base)
        mode = int(g.integers(0, 4))
        bits[base:base + m] = (np.zeros(m, bool), g.random(m) < 0.15, g.random(m) < 0.5, np.ones(m, bool))[mode]
    return bits


def full_blocks(name):
    w, _, n = trace_rows(name)
    groups = _chunks(np.arange(len(w)))
    return Blocks(name, groups, np.tile(words_of(np.ones(n, bool)), (len(groups), 1)))


@functools.lru_cache(maxsize=None)
def prefix_blocks(name, seed=41):
    """Rows sorted by the primitive the oracle finds; a block of 64 keeps every primitive up to the largest one its rows hit, and random ones
    above.  The oracle takes the first of equally distant primitives in list order (strict '<', src/scene.cpp:433-445), so with every
    lower-indexed primitive kept the winner of each row is kept and stays the winner.  Rows that hit nothing get blocks of their own with
    masks that are random throughout."""
    _, ref, n = trace_rows(name)
    g = np.random.default_rng(seed)
    hp = ref[:, 0]
    order = np.argsort(hp, kind="stable")
    hits, misses = order[hp[order] != MISS], order[hp[order] == MISS]
    groups, masks = [], []
    for blk in _chunks(hits):
        bits = _random_bits(g, n)
        bits[:int(hp[blk].max()) + 1] = True
        groups.append(blk); masks.append(words_of(bits))
    for blk in _chunks(misses):
        groups.append(blk); masks.append(words_of(_random_bits(g, n)))
    return Blocks(name, groups, masks)


@functools.lru_cache(maxsize=None)
def masked_out_blocks(name):
    """Rows sorted by the primitive the oracle finds (and by the primitive they ignore); a block keeps everything EXCEPT the primitives its
    rows hit.  `single` [64 * blocks]: the one primitive the block leaves out, -1 where it leaves out several or none."""
    w, ref, n = trace_rows(name)
    hp = ref[:, 0]
    order = np.lexsort((w[:, 6].view(np.int32), hp))
    groups, masks, single = [], [], []
    for blk in _chunks(order[hp[order] != MISS]):
        out = np.unique(hp[blk])
        bits = np.ones(n, dtype=bool)
        bits[out] = False
        groups.append(blk); masks.append(words_of(bits))
        single += [int(out[0]) if len(out) == 1 else -1] * 64
    b = Blocks(name, groups, masks)
    b.single = np.array(single, dtype=np.int64)
    return b


def coverage(blocks):
    """What the masks of `blocks` put into the masked pass 1, read from the masks themselves: (the places (group, q) with q in WATCHED_Q at which
    some block keeps a primitive, the places that exist in the scene, the groups some block leaves empty)"""
    n = trace_rows(blocks.name)[2]
    kept = tm.unpack(blocks.masks, n)                     # [blocks, n]
    exist = {(q >> 5, q & 31) for q in range(n) if (q & 31) in WATCHED_Q}
    seen = {(q >> 5, q & 31) for q in range(n) if (q & 31) in WATCHED_Q and kept[:, q].any()}
    empty = {base >> 5 for base in range(0, n, 32) if (~kept[:, base:base + 32].any(axis=1)).any()}
    return seen, exist, empty


# ---- whole samples in the mode the calibration does not choose ----------------------------------------------------------------------------
SAMPLE_RES, SAMPLE_SPP = (24, 20), 3
SAMPLE_CASES = ("prims33", "prims70", "prims128-2006", "triangles", "degenerate-room", "shared-edge") + tuple("random-%d" % s for s in range(6))
DEFAULT_FLAGS = dict(indirect_only=False, els=True, flat_field=True)


def sample_case(name):
    """(scene, render flags for Oracle.samples / Oracle.render, seed)"""
    if name.startswith("random-"):
        seed = int(name.split("-")[1])
        c, flags = crafted.random_scene(seed)
        return c, flags, seed
    c = {"prims33": lambda: crafted.many_prims_scene(33), "prims70": lambda: crafted.many_prims_scene(70),
         "prims128-2006": lambda: crafted.many_prims_scene(128, 2006), "triangles": crafted.triangle_scene,
         "degenerate-room": lambda: crafted.degenerate_light_scene("room"), "shared-edge": crafted.shared_edge_scene}[name]()
    return c, dict(DEFAULT_FLAGS), 5
