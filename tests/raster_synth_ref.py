"""Synthetic meshes for the rasteriser's rarely taken branches, and the margin rule (TEST INFRASTRUCTURE ONLY).

The seven render launches share one body (csrc/so100_render.h).  The real scene never fills the phase-B list, never
drops a triangle at the near plane and has no exact depth ties, and its tests allow 1 % of the pixels to differ.  The
meshes here reach those branches, and the GPU is held to the float64 restatements (render_ref, render_aux_ref,
render_msaa_ref) EXACTLY on every pixel that is KEPT.  A pixel is kept when, judged from float64 alone,

* for every triangle whose box of pixels holds it, the pixel centre (with S samples: each sample point) is more than
  DELTA pixels from each of the triangle's three edge lines, and
* the two nearest depths at the pixel (at each sample) differ by more than EPS, relative.

The meshes of the EXACT cases are dyadic: with fovy 90, a dyadic aspect (128x64), the camera at the origin and
power-of-two inverse depths every screen coordinate and edge function is exact in float32 (test_raster_synth_cpu.py
asserts that the float32 set-up lies on a 1/1024 grid and is the float64 one rounded), so every pixel is kept, those on
an edge and the exact ties included.  Their reference is the float32 restatement: with every operation exact it is the
rules in real arithmetic, whereas float64 numpy's tan(pi / 4) is 1 - 1.1e-16 and moves an edge off the pixel centres.

Measured by tests/test_raster_synth_cpu.py (float32 numpy on the float32 oracle's frames against float64 on the
float64 oracle's, all non-exact cases; the smallest values at which the two agree on every kept pixel):

    DELTA_MEASURED = 0 px, EPS_MEASURED = 0 (float32 numpy flips no pixel of these images), DEPTH_REL_MEASURED = 7.3e-06

The tests use FACTOR = 4 times those (the GPU contracts FMAs and its tanf is not numpy's).  A measured 0 is no margin,
so each has a floor from the number format: a screen coordinate is the end of a chain of 6 float32 roundings at a
magnitude under 256 px, 6 x half a spacing of 2^-16 px = 4.6e-5 px (DELTA_FLOOR), and DELTA = 4 x max(measured, floor)
= 1.83e-4 px; two depths that are each within DEPTH_REL_BAR of their value can change order only when they are closer
than twice that, so EPS = max(4 x measured, 2 x DEPTH_REL_BAR) = 5.84e-5; DEPTH_REL_BAR = 4 x 7.3e-6 = 2.92e-5.  Left out
at those: at most 0.9 % of an image's pixels (cap 5 %) and 0 % of a multisampled image's (cap 10 %).

Colours are unique per triangle and the lighting is flat (head_ambient 1, nothing else), so a pixel's colour names its
winning triangle: colour-exact is winner-exact.
"""
import ctypes

import numpy as np

import render_aux_ref as A
import render_msaa_ref as M
import render_ref

NBODY, CUBE, LINK = 9, 8, 4
N_ENVS = 3
FACTOR = 4.0
DELTA_MEASURED, EPS_MEASURED, DEPTH_REL_MEASURED = 0.0, 0.0, 7.3e-6
DELTA_FLOOR = 6 * 0.5 * 2.0 ** -16
DELTA = FACTOR * max(DELTA_MEASURED, DELTA_FLOOR)
DEPTH_REL_BAR = FACTOR * DEPTH_REL_MEASURED
EPS = max(FACTOR * EPS_MEASURED, 2 * DEPTH_REL_BAR)
SHARE_CAP, SHARE_CAP_MSAA = 0.05, 0.10
# csrc/so100_render.h
TILE_PX, BIG_PX, BIG_CAP, BIG_CAP_MSAA, WIDE_KEYS, THREADS = 4096, 64, 256, 1024, 1024, 256
MID_CAP = BIG_CAP_MSAA - BIG_CAP
CUBE_POS = (0.25, -0.125, -0.5)
# the five materials' colours of the launches with view records (packed RGB8)
PALETTE = np.array([0x2040E0, 0x40C020, 0xE06010, 0x8080F0, 0xF0F040], np.uint32)
ZNEAR = 2.0 ** -7
ZNEAR_TINY = 2.0 ** -20


def qpos():
    """float32 [3, 13]: three arm poses; the cube at CUBE_POS with the identity quaternion in every env (a camera
    mounted on it is then one world camera for all envs)."""
    q = np.zeros((N_ENVS, 13), np.float32)
    q[1, :6] = [0.5, -0.3, 0.4, -0.2, 0.6, 0.1]
    q[2, :6] = [-0.7, 0.2, -0.5, 0.3, -0.4, 0.25]
    q[:, 6:9] = CUBE_POS
    q[:, 9] = 1.0
    return q


def frames(oracle, model):
    """[env] of [NBODY] of (R, p): the oracle's body frames at qpos()."""
    return [A.frames_of(oracle, model, q.astype(np.float64))[0] for q in qpos()]


def camera(znear=ZNEAR, pos=(0.0, 0.0, 0.0), lights=None):
    """render_ref.camera_dict's dict of the hand-made camera: at `pos` looking along the world's -z (mat = identity),
    fovy 90, no tracking, flat lighting; lights = (dirs, diffuses, head_ambient, head_diffuse) for the lit case."""
    cam = {"pos": np.array(pos, np.float64), "mat": np.eye(3), "track": 0, "fovy": 90.0, "znear": float(znear),
           "head_ambient": 1.0, "head_diffuse": 0.0, "light_dir": [], "light_diffuse": []}
    if lights is not None:
        dirs, diff, amb, hd = lights
        cam.update(light_dir=[np.array(d, np.float64) for d in dirs], light_diffuse=[float(c) for c in diff],
                   head_ambient=float(amb), head_diffuse=float(hd))
    return cam


def camera_struct(cam, pos=None):
    """so100_camera of a camera dict (pos: another position, e.g. in a body's frame)."""
    from gym_so100 import _native
    c = _native.SO100Camera()
    c.pos[:] = [float(x) for x in (cam["pos"] if pos is None else pos)]
    c.mat[:] = [float(x) for x in np.asarray(cam["mat"]).reshape(-1)]
    c.track, c.fovy, c.znear = 0, cam["fovy"], cam["znear"]
    c.head_ambient, c.head_diffuse = cam["head_ambient"], cam["head_diffuse"]
    c.nlight = len(cam["light_dir"])
    for i, (d, k) in enumerate(zip(cam["light_dir"], cam["light_diffuse"])):
        c.light_dir[i][:] = [float(x) for x in d]
        c.light_diffuse[i] = k
    return c


def view_words(cam, n, pos=None):
    """int32 [n, 40]: n identity so100_view records of the camera with PALETTE as the materials' colours."""
    from gym_so100 import _native
    v = _native.SO100View()
    v.pos[:] = [float(x) for x in (cam["pos"] if pos is None else pos)]
    v.mat[:] = [float(x) for x in np.asarray(cam["mat"]).reshape(-1)]
    v.fovy, v.head_ambient, v.head_diffuse = cam["fovy"], cam["head_ambient"], cam["head_diffuse"]
    for i, (d, k) in enumerate(zip(cam["light_dir"], cam["light_diffuse"])):
        v.light_dir[i][:] = [float(x) for x in d]
        v.light_diffuse[i] = k
    v.rgb[:] = [int(x) for x in PALETTE]
    w = np.frombuffer(ctypes.string_at(ctypes.byref(v), ctypes.sizeof(v)), np.int32)
    return np.ascontiguousarray(np.tile(w, (n, 1)))


# ------------------------------------------------------------------------------------------------------- meshes
def unproject(sx, sy, depth, W, H):
    """World points (float64 [..., 3]) that the origin camera (fovy 90, mat identity) sees at screen (sx, sy), depth."""
    sx, sy, depth = np.broadcast_arrays(*(np.asarray(v, np.float64) for v in (sx, sy, depth)))
    x = (sx / W - 0.5) * 2.0 * (W / H) * depth
    y = (0.5 - sy / H) * 2.0 * depth
    return np.stack([x, y, -depth], axis=-1)


def unique_rgb(T, first=0):
    """(rgb float32 [T, 3], packed uint32 [T]): a distinct non-zero RGB8 per triangle, as byte / 255."""
    q = ((np.arange(first, first + T, dtype=np.uint64) + np.uint64(1)) * np.uint64(2654435761)) & np.uint64(0xFFFFFF)
    q = q.astype(np.uint32)
    rgb = np.stack([(q >> (8 * k)) & 0xFF for k in range(3)], axis=-1).astype(np.float32) / np.float32(255)
    return rgb, q


def rgb_of(packed):
    q = np.asarray(packed, np.uint32)
    return np.stack([(q >> (8 * k)) & 0xFF for k in range(3)], axis=-1).astype(np.float32) / np.float32(255)


def make_mesh(world, body=None, rgb=None, label=None, link_frame=None):
    """world: float64 [T, 3, 3] world vertices as env 0 sees them; body [T] (default the world): a cube triangle is
    stored relative to CUBE_POS, an arm-link triangle in `link_frame` (env 0's (R, p) of body LINK)."""
    world = np.asarray(world, np.float64)
    T = len(world)
    body = np.zeros(T, np.int32) if body is None else np.asarray(body, np.int32)
    local = world.copy()
    local[body == CUBE] -= np.array(CUBE_POS)
    if np.any(body == LINK):
        R, p = link_frame
        local[body == LINK] = (world[body == LINK] - p) @ R             # R^T (w - p)
    rgb = unique_rgb(T)[0] if rgb is None else np.asarray(rgb, np.float32)
    label = (np.arange(T) * 7 % 251).astype(np.uint8) if label is None else np.asarray(label, np.uint8)
    return {"tri": np.ascontiguousarray(local, np.float32), "body": np.ascontiguousarray(body),
            "rgb": np.ascontiguousarray(rgb), "label": np.ascontiguousarray(label),
            "material": np.ascontiguousarray(np.arange(T) % 5, np.uint8)}


def reversed_mesh(mesh):
    return {k: np.ascontiguousarray(v[::-1]) for k, v in mesh.items()}


def subset_mesh(mesh, keep):
    return {k: np.ascontiguousarray(v[keep]) for k, v in mesh.items()}


def palette_mesh(mesh):
    """The mesh as a launch with view records colours it: the base colour is PALETTE[material]."""
    return dict(mesh, rgb=rgb_of(PALETTE[mesh["material"]]))


def random_mesh(W, H, T, seed, link_frame):
    """T random triangles of +-8 to +-16 px about centres across the image, sloped, at depths 1..3: 70 % on the world,
    15 % on the cube, 15 % on arm link LINK."""
    rng = np.random.default_rng(seed)
    c = np.stack([rng.uniform(-8, W + 8, T), rng.uniform(-8, H + 8, T)], axis=-1)
    s = rng.uniform(8, 16, T)
    v = c[:, None, :] + rng.uniform(-1, 1, (T, 3, 2)) * s[:, None, None]
    d = rng.uniform(1, 3, T)[:, None] * (1 + rng.uniform(-0.1, 0.1, (T, 3)))
    u = rng.uniform(0, 1, T)
    body = np.where(u < 0.7, 0, np.where(u < 0.85, CUBE, LINK))
    return make_mesh(unproject(v[..., 0], v[..., 1], d, W, H), body=body, link_frame=link_frame)


def corner_triangles(cells, legs, W, H, d0=2.0, step=1.0 / 1024):
    """Right triangles with the right angle at the integer screen points `cells` [(x0, y0)] and legs of `legs` px along
    +x and +y, at constant depths that fall by `step` per triangle: a later one is nearer.  With the cells in raster
    order no later triangle reaches an earlier one's corner pixels, so triangle i wins at least the cell at its
    corner, however many others its box and its area overlap."""
    cells = np.asarray(cells, np.float64)
    legs = np.broadcast_to(np.asarray(legs, np.float64), (len(cells),))
    x0, y0 = cells[:, 0], cells[:, 1]
    sx = np.stack([x0, x0 + legs, x0], axis=-1)
    sy = np.stack([y0, y0, y0 + legs], axis=-1)
    d = (d0 - step * np.arange(len(cells)))[:, None] * np.ones((1, 3))
    return unproject(sx, sy, d, W, H)


def band_rows(W, S=1):
    return max(1, TILE_PX // (W * S))


def overflow_mesh(W, H, count, cell=2, leg=256.0):
    """`count` corner triangles whose legs leave the image (each covers the whole quadrant right of and below its
    corner), on the cells of `cell` x `cell` px of band 0 in raster order, each cell chosen so that the triangle's box in
    band 0 is well over kBigPx (>= 80 px): band 0's list holds exactly `count`, and triangle i wins its cell's
    cell^2 pixels, all of them at least 0.5 px from every edge line."""
    rows = min(H, band_rows(W))
    cells = [(x, y) for y in range(0, rows - cell + 1, cell) for x in range(0, W - cell + 1, cell)
             if (W - x + 1) * (rows - y + 1) >= 80 and (W - x) * (rows - y) >= 80]
    assert len(cells) >= count, (W, H, len(cells), count)
    # spread over the band: every n-th valid cell, so the last rows are used by the small meshes too
    pick = [cells[i * len(cells) // count] for i in range(count)]
    return make_mesh(corner_triangles(pick, leg, W, H))


def msaa_overflow_mesh(W, H, S, offsets, nwide, nmid):
    """Corner triangles on the pixels of band 0 (S samples per pixel) in raster order, nwide of them with a box of at
    least 1.1 kWideKeys keys in the band and nmid with a box between 1.1 kBigPx and 0.9 kWideKeys keys: the leg decides
    the box, the corner pixel (all of its samples) is the triangle's own.  Wide and mid ones alternate along the raster
    order in proportion."""
    rows = min(H, band_rows(W, S))
    off = np.asarray(offsets, np.float64)
    oxlo, oxhi, oylo, oyhi = off[:, 0].min(), off[:, 0].max(), off[:, 1].min(), off[:, 1].max()

    def keys(x, y, leg):
        bx0, bx1 = max(0, int(np.floor(x - 0.5 - oxhi))), min(W - 1, int(np.ceil(x + leg - 0.5 - oxlo)))
        by0, by1 = max(0, int(np.floor(y - 0.5 - oyhi))), min(rows - 1, int(np.ceil(y + leg - 0.5 - oylo)))
        return (bx1 - bx0 + 1) * (by1 - by0 + 1) * S
    cells, legs, kind = [], [], []
    want = {"wide": nwide, "mid": nmid}
    have = {"wide": 0, "mid": 0}
    for y in range(rows):
        for x in range(W):
            # the wide ones are spread over the upper half of the band, where a box can still be that large
            due = have["wide"] < want["wide"] * min(1.0, (y * W + x + 1) / (0.5 * rows * W))
            order = ("wide", "mid") if due else ("mid", "wide")
            for k in order:
                if have[k] >= want[k]:
                    continue
                if k == "wide":
                    leg = next((L for L in (24.0, 32.0, 48.0, 64.0, 128.0) if keys(x, y, L) >= 1.1 * WIDE_KEYS), None)
                else:
                    leg = next((L for L in (6.0, 4.0, 3.0, 8.0, 2.0) if 1.1 * BIG_PX <= keys(x, y, L) <= 0.9 * WIDE_KEYS),
                               None)
                if leg is not None:
                    cells.append((x, y)); legs.append(leg); kind.append(k); have[k] += 1
                    break
    assert have == want, (W, H, S, have, want)
    return make_mesh(corner_triangles(cells, legs, W, H, step=1.0 / 2048))


def near_mesh(W, H, znear):
    """Triangles against the near plane, on the world body under the origin camera (a vertex's depth is -z, exact).
    Triangle k < 9 has two vertices at depth 1 in column k of the image's left part; its third vertex decides:
    0 beyond (drawn); 1 exactly at znear; 2 one ulp inside; 3 one ulp beyond (drawn); 4 two vertices inside; 5 all three
    inside; 6 wholly behind the camera; 7 one vertex behind the camera; 8 one vertex at depth 0.  9 and 10 have a vertex
    one ulp beyond znear far off the axis: screen coordinates of ~1e7 and ~6e8 px, for the box clamp and the
    float-to-int conversion.  An edge function based at such a vertex resolves a pixel's position to the float32
    spacing there (2 and 64 px), so their coverage cannot be graded: they lie under 11, an occluder in front of the
    image's right part, and must not show.  12 is a backdrop over the whole image at depth 2.
    Returns (mesh, beyond, visible): whether triangle k passes the near plane, and whether it wins any pixel."""
    zn = np.float32(znear)
    up, dn = float(np.nextafter(zn, np.float32(1))), float(np.nextafter(zn, np.float32(0)))
    zn = float(zn)
    assert dn < zn < up

    def col(k, third, second=None, x=None):
        x = 3.0 + 6.0 * k if x is None else x
        a = unproject(x, 20.0, 1.0, W, H)
        b = unproject(x + 4.0, 24.0, 1.0, W, H) if second is None else second
        return np.stack([a, b, np.asarray(third, np.float64)])
    tri = [col(0, unproject(8.0, 50.0, 1.25, W, H)),
           col(1, [0.0, -0.25 * zn, -zn]),
           col(2, [0.0, -0.25 * dn, -dn]),
           col(3, [-0.5 * up, -0.5 * up, -up]),
           col(4, [0.0, -0.001, -dn], second=np.array([0.001, 0.0, -0.5 * zn])),
           np.array([[0.0, 0.0, -0.5 * zn], [1e-4, 0.0, -0.25 * zn], [0.0, 1e-4, -dn]]),
           unproject([10.0, 40.0, 25.0], [30.0, 30.0, 45.0], -1.0, W, H),
           col(7, [0.0, -1.0, 1.0]),
           col(8, [0.0, -1.0, 0.0]),
           col(0, [0.25, -0.5, -up], x=72.0),
           col(0, [16.0, -8.0, -up], x=80.0),
           unproject([58.0, 200.0, 58.0], [-100.0, -100.0, 300.0], 2.0 ** -6, W, H),
           unproject([-W, 3.0 * W, -W], [-H, -H, 3.0 * H], 2.0, W, H)]
    beyond = np.array([1, 0, 0, 1, 0, 0, 0, 0, 0, 1, 1, 1, 1], bool)
    visible = np.array([1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 1], bool)
    return make_mesh(np.stack(tri)), beyond, visible


def _dy(sx, sy, iz, W=128, H=64):
    """An exact triangle: screen vertices on a dyadic grid, inverse depths powers of two."""
    return unproject(np.asarray(sx, np.float64), np.asarray(sy, np.float64), 1.0 / np.asarray(iz, np.float64), W, H)


def ties_mesh(single=False):
    """Exact duplicates at 128x64 (dyadic, see the module docstring).  Group g is one triangle stated several times:
    different colours in both mesh orders, the other winding, a cyclic shift of the vertices, three copies, and for the
    aux key the same colour with different labels in both orders.  single=True: the first copy of each group alone.
    Returns (mesh, expect) with expect = [(x, y, packed colour, label)], a pixel inside each group and what wins it."""
    big, small = 0xF0E0D0, 0x102030
    groups = [
        (([4.5, 28.5, 8.5], [4.5, 8.5, 26.5], [1.0, 0.5, 0.25]),
         [((0, 1, 2), big, 9), ((0, 1, 2), small, 9)]),
        (([34.5, 58.5, 38.5], [4.5, 8.5, 26.5], [1.0, 0.5, 0.25]),
         [((0, 1, 2), small, 9), ((0, 1, 2), big, 9)]),
        (([64.5, 88.5, 68.5], [4.5, 8.5, 26.5], [0.5, 0.5, 1.0]),
         [((0, 1, 2), big, 9), ((0, 2, 1), small, 9), ((1, 2, 0), 0x808080, 9)]),
        (([94.5, 118.5, 98.5], [4.5, 8.5, 26.5], [0.5, 0.25, 0.5]),
         [((0, 1, 2), 0x4060A0, 7), ((2, 1, 0), 0x4060A0, 3), ((1, 2, 0), 0x4060A0, 5)]),
        # across the band boundary (rows 31 | 32) and with a sloped depth
        (([10.25, 50.75, 20.5], [28.5, 30.25, 40.75], [1.0, 0.25, 0.5]),
         [((0, 1, 2), 0x00FF00, 200), ((1, 0, 2), 0x00FE00, 100), ((2, 0, 1), 0x01FE00, 1)]),
        (([70.5, 110.5, 90.5], [36.5, 36.5, 60.5], [0.25, 0.25, 0.25]),
         [((0, 1, 2), 0x0000FF, 4), ((0, 1, 2), 0x0000FF, 2), ((0, 1, 2), 0x0000FF, 250)]),
    ]
    tri, rgb, lab, expect = [], [], [], []
    for (sx, sy, iz), copies in groups:
        base = _dy(sx, sy, iz)
        for order, colour, label in (copies[:1] if single else copies):
            tri.append(base[list(order)]); rgb.append(colour); lab.append(label)
        cs = copies[:1] if single else copies
        wc = min(c[1] for c in cs)
        expect.append((int(np.mean(sx)), int(np.mean(sy)), wc, min(c[2] for c in cs if c[1] == wc)))
    return make_mesh(np.stack(tri), rgb=rgb_of(rgb), label=lab), expect


def edges_mesh():
    """Exact edge and reject cases at 128x64 (two bands of 32 rows): shared edges through pixel centres (vertical,
    horizontal on the band boundary's rows, diagonal), zero-area triangles, slivers between pixel centres, boxes wholly
    outside the image on each side, triangles across the band boundary, and one that fills the image behind all."""
    T = []
    T.append(_dy([-128, 384, -128], [-64, -64, 192], [0.25, 0.25, 0.25]))          # fills the image
    # the pairs below share an edge through pixel centres and are mirror images across it: equal |area| and equal
    # weights on the edge, so both give its pixels the same depth bits and the key decides.  (The kernel multiplies by
    # 1 / area where the restatement divides: two coplanar triangles of different areas may differ in the last bit)
    # a kite split along x = 20.5, outer edges through centres too
    T.append(_dy([8.5, 20.5, 20.5], [10.5, 2.5, 18.5], [1, 1, 1]))
    T.append(_dy([32.5, 20.5, 20.5], [10.5, 18.5, 2.5], [1, 1, 1]))
    # a square split along its diagonal through centres; the two halves at the same depth
    T.append(_dy([40.5, 56.5, 56.5], [4.5, 4.5, 20.5], [0.5, 0.5, 0.5]))
    T.append(_dy([40.5, 56.5, 40.5], [4.5, 20.5, 20.5], [0.5, 0.5, 0.5]))
    # shared horizontal edge on row 31's centres (y = 31.5, the last row of band 0) and one on row 32's (y = 32.5)
    T.append(_dy([64.5, 90.5, 76.5], [31.5, 31.5, 22.5], [1, 1, 0.5]))
    T.append(_dy([64.5, 90.5, 76.5], [31.5, 31.5, 40.5], [1, 1, 0.5]))
    T.append(_dy([96.5, 120.5, 108.5], [32.5, 32.5, 26.5], [0.5, 1, 1]))
    T.append(_dy([96.5, 120.5, 108.5], [32.5, 32.5, 38.5], [0.5, 1, 1]))
    # across the band boundary: a tall one, one ending exactly on y = 32 (between the rows) from above and from below
    T.append(_dy([4.25, 16.75, 9.5], [24.25, 29.5, 58.75], [1, 0.5, 1]))
    T.append(_dy([24.5, 44.5, 34.5], [26.5, 32.0, 32.0], [1, 1, 1]))
    T.append(_dy([24.5, 44.5, 34.5], [38.5, 32.0, 32.0], [1, 1, 1]))
    # zero area: collinear, and a repeated vertex
    T.append(_dy([50.5, 54.5, 58.5], [40.5, 44.5, 48.5], [1, 1, 1]))
    T.append(_dy([60.5, 60.5, 70.5], [50.5, 50.5, 55.5], [1, 1, 1]))
    # slivers between pixel centres (vertical, horizontal) and one that holds exactly one column of centres
    T.append(_dy([50.625, 50.875, 50.75], [50.0, 50.0, 62.0], [1, 1, 1]))
    T.append(_dy([70.0, 70.0, 90.0], [58.625, 58.875, 58.75], [1, 1, 1]))
    T.append(_dy([100.25, 100.75, 100.5], [44.0, 44.0, 62.0], [1, 1, 1]))
    # wholly outside: left, right, above, below; and partly outside at the corners
    T.append(_dy([-20.5, -0.75, -10.5], [10.5, 20.5, 30.5], [1, 1, 1]))
    T.append(_dy([128.75, 150.5, 140.5], [10.5, 20.5, 30.5], [1, 1, 1]))
    T.append(_dy([30.5, 60.5, 40.5], [-30.5, -0.75, -10.5], [1, 1, 1]))
    T.append(_dy([30.5, 60.5, 40.5], [64.75, 80.5, 70.5], [1, 1, 1]))
    T.append(_dy([-6.5, 6.5, -6.5], [-6.5, -6.5, 6.5], [1, 1, 1]))
    T.append(_dy([134.5, 121.5, 134.5], [70.5, 70.5, 57.5], [1, 1, 1]))
    return make_mesh(np.stack(T))


def grid_mesh(count):
    """`count` small exact triangles at 128x64 on a grid of 8 x 8 px cells (count = 257: one more than the threads)."""
    T = []
    for i in range(count):
        x, y = 8.0 * (i % 16) + 0.25 * (i // 128), 4.0 * ((i // 16) % 16)
        T.append(_dy([x + 0.5, x + 6.5, x + 2.5], [y + 0.25, y + 1.5, y + 3.75], [1, 1, 0.5]))
    return make_mesh(np.stack(T))


_CASES = {}
# the cases' names, known without building a mesh (the GPU tests are parametrised by them)
SINGLE = (("random_96x72", "random_129x33", "lit_96x72") +
          tuple(f"overflow{c}_{w}x{h}" for w, h in ((96, 72), (129, 33)) for c in (255, 256, 257, 768)) +
          ("near_96x72", "ties", "ties_reversed", "ties_single", "edges", "one", "n257"))
MULTI = (tuple(f"msaa_{t}_{w}x{h}x{s}" for w, h, s in ((64, 48, 4), (128, 32, 2)) for t in ("wide", "mid", "under")) +
         ("ties_msaa4", "ties_reversed_msaa4", "edges_msaa4", "n257_msaa4", "edges_msaa2"))


def cases(link_frame):
    """{name: case}: case = dict(mesh, cam, W, H, msaa (offsets or None), exact, kind, ...).  link_frame: env 0's
    (R, p) of body LINK from the float64 oracle."""
    if _CASES:
        return _CASES
    flat, tiny = camera(ZNEAR), camera(ZNEAR_TINY)

    def add(name, mesh, W, H, cam=flat, msaa=None, exact=False, kind="random", **kw):
        _CASES[name] = dict(name=name, mesh=mesh, cam=cam, W=W, H=H, msaa=msaa, exact=exact, kind=kind, **kw)
    add("random_96x72", random_mesh(96, 72, 1200, 1, link_frame), 96, 72, shift=(0.125, 0.0, 0.0))
    add("random_129x33", random_mesh(129, 33, 800, 2, link_frame), 129, 33)
    lights = ([(0.0, 0.6, -0.8), (-0.57735, 0.57735, -0.57735)], [0.4, 0.3], 0.3, 0.5)
    add("lit_96x72", random_mesh(96, 72, 600, 3, link_frame), 96, 72, cam=camera(ZNEAR, lights=lights), kind="lit")
    for W, H in ((96, 72), (129, 33)):
        for count in (255, 256, 257, 3 * 256):
            add(f"overflow{count}_{W}x{H}", overflow_mesh(W, H, count), W, H, kind="overflow", count=count)
    for W, H, S, off in ((64, 48, 4, M.ROTATED4), (128, 32, 2, M.DIAG2)):
        for tag, nw, nm in (("wide", 262, 40), ("mid", 12, 774), ("under", 250, 760)):
            if S == 4 and tag == "under":
                nw, nm = 250, 700                                    # a 64 x 16 band has 1024 corner pixels in all
            add(f"msaa_{tag}_{W}x{H}x{S}", msaa_overflow_mesh(W, H, S, off, nw, nm), W, H, msaa=off, kind="msaa_overflow",
                nwide=nw, nmid=nm)
    mesh, beyond, visible = near_mesh(96, 72, ZNEAR_TINY)
    add("near_96x72", mesh, 96, 72, cam=tiny, kind="near", beyond=beyond, visible=visible)
    mesh, expect = ties_mesh()
    add("ties", mesh, 128, 64, exact=True, kind="ties", expect=expect)
    add("ties_reversed", reversed_mesh(mesh), 128, 64, exact=True, kind="ties", expect=expect)
    add("ties_single", ties_mesh(single=True)[0], 128, 64, exact=True, kind="ties_single")
    add("edges", edges_mesh(), 128, 64, exact=True, kind="edges")
    add("one", grid_mesh(1), 128, 64, exact=True, kind="edges")
    add("n257", grid_mesh(257), 128, 64, exact=True, kind="edges")
    for name in ("ties", "ties_reversed", "edges", "n257"):
        c = _CASES[name]
        add(name + "_msaa4", c["mesh"], 128, 64, msaa=M.ROTATED4, exact=True, kind=c["kind"])
    add("edges_msaa2", _CASES["edges"]["mesh"], 128, 64, msaa=M.DIAG2, exact=True, kind="edges")
    return _CASES


# ------------------------------------------------------------------------------------- projection, boxes, margins
def project(mesh, frames, cam, W, H, dtype=np.float64):
    """The restatements' set-up in `dtype` arithmetic, operation for operation: (sx, sy, iz [T, 3], ok [T])."""
    dt = np.dtype(dtype).type
    pos, mat = np.asarray(cam["pos"], dt), np.asarray(cam["mat"], dt)
    R = np.stack([f[0] for f in frames]).astype(dt)[mesh["body"]]
    P = np.stack([f[1] for f in frames]).astype(dt)[mesh["body"]]
    w = np.einsum("tij,tvj->tvi", R, mesh["tri"].astype(dt)) + P[:, None, :]
    c = (w - pos) @ mat
    depth = -c[..., 2]
    th = np.tan(dt(0.5) * np.radians(dt(cam["fovy"])))
    aspect = dt(W) / dt(H)
    ok = np.all(depth > dt(cam["znear"]), axis=1)
    with np.errstate(all="ignore"):
        iz = dt(1.0) / np.where(depth > 0, depth, dt(1.0))
        sx = (c[..., 0] * iz / (th * aspect) * dt(0.5) + dt(0.5)) * dt(W)
        sy = (dt(0.5) - c[..., 1] * iz / th * dt(0.5)) * dt(H)
    return sx, sy, iz, ok


def _extremes(offsets, dt):
    off = np.asarray(((0.0, 0.0),) if offsets is None else offsets, np.float64).astype(dt)
    return off, off[:, 0].min(), off[:, 0].max(), off[:, 1].min(), off[:, 1].max()


def boxes(sx, sy, ok, W, y0, y1, offsets=None, dtype=np.float64):
    """The kernel's box of pixels of every triangle in the band of rows [y0, y1): int [T, 4] (bx0, bx1, by0, by1) and
    live [T]: beyond znear, |area| > 1e-12, a non-empty box."""
    dt = np.dtype(dtype).type
    off, oxlo, oxhi, oylo, oyhi = _extremes(offsets, dt)
    half = dt(0.5)
    with np.errstate(all="ignore"):
        area = (sx[:, 1] - sx[:, 0]) * (sy[:, 2] - sy[:, 0]) - (sx[:, 2] - sx[:, 0]) * (sy[:, 1] - sy[:, 0])
        lo = lambda v: np.clip(np.nan_to_num(np.floor(v), nan=0.0, posinf=2e9, neginf=-2e9), -2e9, 2e9).astype(np.int64)
        bx0 = np.maximum(0, lo(sx.min(axis=1) - half - oxhi))
        bx1 = np.minimum(W - 1, lo(np.ceil(sx.max(axis=1) - half - oxlo)))
        by0 = np.maximum(y0, lo(sy.min(axis=1) - half - oyhi))
        by1 = np.minimum(y1 - 1, lo(np.ceil(sy.max(axis=1) - half - oylo)))
    live = ok & (np.abs(area) > 1e-12) & (bx0 <= bx1) & (by0 <= by1)
    return np.stack([bx0, bx1, by0, by1], axis=-1), live


def list_counts(case, frames, dtype=np.float64):
    """Per band: the triangles phase A lists.  Single sample: [(rows, listed indices)]; multisampled:
    [(rows, wide indices, mid indices)].  Also asserts that no box is within 10 % of a threshold (25 % of kBigPx for
    the single-sample meshes)."""
    W, H, off = case["W"], case["H"], case["msaa"]
    S = 1 if off is None else len(off)
    sx, sy, iz, ok = project(case["mesh"], frames, case["cam"], W, H, dtype)
    rows = band_rows(W, S)
    out = []
    for y0 in range(0, H, rows):
        y1 = min(H, y0 + rows)
        b, live = boxes(sx, sy, ok, W, y0, y1, off, dtype)
        keys = (b[:, 1] - b[:, 0] + 1) * (b[:, 3] - b[:, 2] + 1) * S
        keys = np.where(live, keys, 0)
        if off is None:
            out.append(((y0, y1), np.nonzero(keys > BIG_PX)[0], keys))
        else:
            out.append(((y0, y1), np.nonzero(keys >= WIDE_KEYS)[0], np.nonzero((keys > BIG_PX) & (keys < WIDE_KEYS))[0],
                        keys))
    return out


def margins(case, frames):
    """(edge, gap) float64 [H, W] from float64 alone: the least distance in px of the pixel's centre (of any of its
    sample points) to an edge line of any triangle whose box holds the pixel, and the least relative difference of the
    two nearest depths at the pixel (at any of its samples); inf where there is no such triangle / fewer than two."""
    W, H, offsets = case["W"], case["H"], case["msaa"]
    sx, sy, iz, ok = project(case["mesh"], frames, case["cam"], W, H)
    off, oxlo, oxhi, oylo, oyhi = _extremes(offsets, np.float64)
    S = len(off)
    b, live = boxes(sx, sy, ok, W, 0, H, offsets)
    edge = np.full((H, W), np.inf)
    d1, d2 = np.full((S, H, W), np.inf), np.full((S, H, W), np.inf)
    for t in np.nonzero(live)[0]:
        x, y, z = sx[t], sy[t], iz[t]
        bx0, bx1, by0, by1 = b[t]
        area = (x[1] - x[0]) * (y[2] - y[0]) - (x[2] - x[0]) * (y[1] - y[0])
        cx, cy = np.meshgrid(np.arange(bx0, bx1 + 1) + 0.5, np.arange(by0, by1 + 1) + 0.5)
        sg = 1.0 if area > 0 else -1.0
        sl = (slice(by0, by1 + 1), slice(bx0, bx1 + 1))
        for s in range(S):
            px, py = cx + off[s, 0], cy + off[s, 1]
            w0 = (x[2] - x[1]) * (py - y[1]) - (y[2] - y[1]) * (px - x[1])
            w1 = (x[0] - x[2]) * (py - y[2]) - (y[0] - y[2]) * (px - x[2])
            w2 = (x[1] - x[0]) * (py - y[0]) - (y[1] - y[0]) * (px - x[0])
            dist = np.minimum(np.abs(w0) / np.hypot(x[2] - x[1], y[2] - y[1]),
                              np.minimum(np.abs(w1) / np.hypot(x[0] - x[2], y[0] - y[2]),
                                         np.abs(w2) / np.hypot(x[1] - x[0], y[1] - y[0])))
            edge[sl] = np.minimum(edge[sl], dist)
            izp = (w0 * z[0] + w1 * z[1] + w2 * z[2]) / area
            inside = (w0 * sg >= 0) & (w1 * sg >= 0) & (w2 * sg >= 0) & (izp > 0)
            dep = np.where(inside, 1.0 / np.where(inside, izp, 1.0), np.inf)
            a, c = d1[s][sl], d2[s][sl]
            d2[s][sl] = np.minimum(np.maximum(a, dep), c)
            d1[s][sl] = np.minimum(a, dep)
    with np.errstate(all="ignore"):
        gap = np.where(np.isfinite(d2), (d2 - d1) / d1, np.inf).min(axis=0)
    return edge, gap


def keep_mask(case, edge, gap, delta=DELTA, eps=EPS):
    if case["exact"]:
        return np.ones((case["H"], case["W"]), bool)
    return (edge > delta) & (gap > eps)


# ------------------------------------------------------------------------------------------------ the references
def render(case, frames, dtype=np.float64, mesh=None, cam=None):
    """The restatement's images of one env: dict(rgb, depth, label, win) and, multisampled, rgb_msaa (resolved), smp,
    swin.  depth, label and win are the pixel-centre launch's (the multisampled launch writes colours only)."""
    mesh = case["mesh"] if mesh is None else mesh
    cam = case["cam"] if cam is None else cam
    W, H = case["W"], case["H"]
    rgb, dep, lab, win = A.render(mesh["tri"], mesh["body"], mesh["rgb"], mesh["label"], frames, cam, W, H, dtype=dtype,
                                  winner=True)
    out = dict(rgb=rgb, depth=dep, label=lab, win=win)
    if case["msaa"] is not None:
        res, smp, swin = M.render(mesh["tri"], mesh["body"], mesh["rgb"], frames, cam, W, H, case["msaa"], dtype=dtype,
                                  winner=True)
        out.update(rgb_msaa=res, smp=smp, swin=swin)
    return out


def world_only(mesh):
    return bool(np.all(mesh["body"] == 0))


_REF = {}


def reference(case, frames_list, bits=64, shifted=False):
    """[env] of dict(render()'s images, edge, gap, keep): computed once per (case, arithmetic, camera) and shared (read
    only).  A mesh on the world body alone is the same image in every env.  shifted: from the case's second camera,
    the first moved by case["shift"]."""
    k = (case["name"], bits, shifted)
    if k in _REF:
        return _REF[k]
    cam = case["cam"]
    if shifted:
        cam = dict(cam, pos=np.asarray(cam["pos"]) + np.asarray(case["shift"]))
    c = dict(case, cam=cam)
    out = []
    for fr in frames_list:
        if out and world_only(case["mesh"]):
            out.append(out[0])
            continue
        # an exact case's reference is the float32 restatement: every operation of it is exact, so it is the rules
        # in real arithmetic, whereas float64 numpy's tan(pi / 4) is 1 - 1.1e-16 and moves the dyadic grid by that
        r = render(c, fr, np.float64 if bits == 64 and not case["exact"] else np.float32)
        if bits == 64:
            if case["exact"]:
                r["edge"] = r["gap"] = None
            else:
                r["edge"], r["gap"] = margins(c, fr)
            r["keep"] = keep_mask(case, r["edge"], r["gap"])
        out.append(r)
    _REF[k] = out
    return out


# -------------------------------------------------------------------------------------------- broken restatements
def draw(case, frames, rule=None):
    """A float64 rasteriser of the single-sample rules with one rule broken on request (None: the right rules; its image
    is then render()'s, which test_raster_synth_cpu.py asserts): "near_ge" tests depth >= znear; "clip_vertex" keeps a
    triangle when any of its vertices is beyond znear; "tie_larger" takes the larger colour (then the larger label) on
    equal depths; "exclusive" treats edges as exclusive.  Returns (rgb uint8 [H,W,3], label uint8 [H,W])."""
    W, H, mesh, cam = case["W"], case["H"], case["mesh"], case["cam"]
    # an exact case in float32, as its reference (every operation is exact; the values are then widened)
    sx, sy, iz, ok = (v.astype(np.float64) if v.dtype != bool else v
                      for v in project(mesh, frames, cam, W, H, np.float32 if case["exact"] else np.float64))
    if rule in ("near_ge", "clip_vertex"):
        R = np.stack([f[0] for f in frames])[mesh["body"]]
        P = np.stack([f[1] for f in frames])[mesh["body"]]
        w = np.einsum("tij,tvj->tvi", R, mesh["tri"].astype(np.float64)) + P[:, None, :]
        depth = -((w - cam["pos"]) @ cam["mat"])[..., 2]
        ok = np.all(depth >= cam["znear"], axis=1) if rule == "near_ge" else np.any(depth > cam["znear"], axis=1)
    col = render_ref.pack_rgb(mesh["rgb"])                     # flat lighting: the base colour
    low = (col.astype(np.uint64) << np.uint64(8)) | mesh["label"].astype(np.uint64)
    if rule == "tie_larger":
        low = np.uint64(0xFFFFFFFF) - low
    key = np.full((H, W), A.EMPTY, np.uint64)
    b, live = boxes(sx, sy, ok, W, 0, H)
    for t in np.nonzero(live)[0]:
        x, y, z = sx[t], sy[t], iz[t]
        bx0, bx1, by0, by1 = b[t]
        area = (x[1] - x[0]) * (y[2] - y[0]) - (x[2] - x[0]) * (y[1] - y[0])
        px, py = np.meshgrid(np.arange(bx0, bx1 + 1) + 0.5, np.arange(by0, by1 + 1) + 0.5)
        w0 = (x[2] - x[1]) * (py - y[1]) - (y[2] - y[1]) * (px - x[1])
        w1 = (x[0] - x[2]) * (py - y[2]) - (y[0] - y[2]) * (px - x[2])
        w2 = (x[1] - x[0]) * (py - y[0]) - (y[1] - y[0]) * (px - x[0])
        sg = 1.0 if area > 0 else -1.0
        if rule == "exclusive":
            inside = (w0 * sg > 0) & (w1 * sg > 0) & (w2 * sg > 0)
        else:
            inside = (w0 * sg >= 0) & (w1 * sg >= 0) & (w2 * sg >= 0)
        with np.errstate(all="ignore"):
            izp = (w0 * z[0] + w1 * z[1] + w2 * z[2]) / area
            inside &= izp > 0
            dep = (1.0 / np.where(inside, izp, 1.0)).astype(np.float32)
        k = (dep.view(np.uint32).astype(np.uint64) << np.uint64(32)) | low[t]
        sub = key[by0:by1 + 1, bx0:bx1 + 1]
        np.copyto(sub, np.minimum(sub, k), where=inside)
    empty = key == A.EMPTY
    lo = key & np.uint64(0xFFFFFFFF)
    if rule == "tie_larger":
        lo = np.uint64(0xFFFFFFFF) - lo
    rgb = np.where(empty, np.uint64(0), lo >> np.uint64(8)).astype(np.uint32)
    img = np.stack([(rgb >> (8 * k)) & 0xFF for k in range(3)], axis=-1).astype(np.uint8)
    return img, np.where(empty, np.uint64(255), lo & np.uint64(0xFF)).astype(np.uint8)


def overflow_drops(case, frames):
    """The triangles a kernel that drops what its lists cannot take would lose: per band, the listed ones past the
    list's capacity in index order (the kernel's atomics pick others; every listed triangle is visible, so any choice
    shows)."""
    drop = set()
    for band in list_counts(case, frames):
        if case["msaa"] is None:
            drop.update(band[1][BIG_CAP:].tolist())
        else:
            drop.update(band[1][BIG_CAP:].tolist())
            drop.update(band[2][MID_CAP:].tolist())
    return sorted(drop)
