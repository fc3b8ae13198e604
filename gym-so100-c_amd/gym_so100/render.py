"""Batched camera images on the GPU: the reference's ``so100_pixels_agent_pos`` observation.

The reference renders the ``top`` camera with dm_control's ``physics.render`` on every observation
(gym_so100/tasks/single_arm.py:88-92, env.py:130-136).  ``CameraRenderer`` draws the same camera for
all N envs of an ``SO100VecEnv`` with one HIP launch (csrc/so100_render.hip, C-ABI ``so100_render``):
the scene's visible geoms (assets/so100_render.npz, built by tools/compile_render.py from the
reference MJCF), the camera pose of scene_so100.xml:26-29 (mode="targetbody" on the static table),
fovy 78 and the scene's headlight + three directional lights.  Output: uint8 [N, H, W, 3] on the device, or with
``channels_first`` [N, 3, H, W]; ``render(flat=...)`` also fills a float32 [N, >= 3HW] tensor with the image / 255
in the same launch (C-ABI ``so100_render_to``: one rasterisation, several sinks).

Visual domain randomisation: with ``CameraRenderer.views`` set (a device [N, 40] tensor of ``so100_view`` records,
``identity_views`` / ``sample_views``) env i is drawn from its own camera pose, field of view, lights and material
colours (C-ABI ``so100_render_views``); without it every env is drawn from the one camera, as before.

Depth and segmentation: ``CameraRenderer(depth=True, segmentation=True)`` also keeps ``depth`` (float32 [N, H, W]: metres
along the camera's viewing axis, background 0) and ``segmentation`` (uint8 [N, H, W]: the class of ``segment_labels``,
background ``SEG_BACKGROUND``), what dm_control's ``physics.render(depth=True / segmentation=True)`` returns, written by
the launch that draws the colour image (C-ABI ``so100_render_aux``).

Several cameras: ``MultiCameraRenderer`` draws K <= 4 cameras of every env in one launch whose grid is (env, camera)
(C-ABI ``so100_render_cams``): the reference task's ``top``, ``angle`` and ``front_close`` (tasks/single_arm.py:88-102)
and cameras that ride on a body, such as the arm's own ``left_wrist`` on Fixed_Jaw (so_arm100.xml:126).  ``pixels`` is
[N, K, H, W, 3] (or [N, K, 3, H, W]), depth and segmentation [N, K, H, W], view records [K, N, 40].

Shadows: ``shadows=True`` on either renderer occludes the scene's shadow-casting light (SHADOW_LIGHT, the middle light of
scene_so100.xml:13-16) per pixel by a shadow map that every block builds in LDS inside the one render launch (C-ABI
``so100_render_shadow``): the arm, the jaw and the cube drop hard shadows on the table, the cue a top-down image has for
height.  ``shadow_mask=True`` also keeps ``shadow`` (uint8, 1 = occluded).

Anti-aliasing: ``antialias=True`` (or 2 / 4, or a dict over ``samples`` and ``offsets``) on either renderer draws the
colour images with that many coverage samples per pixel, as the reference scene's 4x multisampled offscreen buffer does
(scene_so100.xml:8, offsamples="4"), resolved in LDS inside the one launch (C-ABI ``so100_render_msaa``).  Depth and
segmentation stay pixel-centre quantities, drawn by a second, aux-only ``so100_render_cams`` launch.

It is a rasteriser of its own, not MuJoCo's OpenGL pipeline: geometry and colours are the scene's, the
pixel values are not MuJoCo's (no specular, shadow filtering or fog, and the sample pattern is not the GL driver's;
DESIGN.md §3.7, §4).
"""
import ctypes
import json
import os

import numpy as np

from . import _native
from .constants import SO100_BOX_SPAWN_RANGES

ASSET = os.path.join(os.path.dirname(os.path.abspath(__file__)), "assets", "so100_render.npz")
CAMERAS = ("top", "angle", "left_pillar", "right_pillar", "front_close")
TRACKING = ("front_close",)              # mode="targetbody" on the ee body: frame per env
# cameras mounted on a body (so100_cams.frame_body): name -> body, position in the body's frame, fovy, tracking.
# left_wrist: so_arm100.xml:126, <camera name="left_wrist" pos="0 .0 0.55" fovy="20" mode="targetbody"
# target="vx300s_left/camera_focus"/> in body Fixed_Jaw (body 6 of 0 world, 1 Base, 2..7 the arm's links, 8 cube)
MOUNTED_CAMERAS = ("left_wrist",)
_MOUNTED = {"left_wrist": dict(body=6, pos=(0.0, 0.0, 0.55), fovy=20.0)}
NBODY = 9
ZNEAR = 0.01
MATERIALS = ("table", "bin", "arm_light", "arm_dark", "cube")      # SO100_NMATERIAL ids 0..4 (include/so100.h)
# segmentation classes (segment_labels): label k is SEG_CLASSES[k], a pixel no triangle covers is SEG_BACKGROUND
SEG_CLASSES = ("table", "bin", "Base", "link1", "link2", "link3", "link4", "link5", "link6", "cube")
SEG_BACKGROUND = 255
# the light that casts shadows: scene_so100.xml:13-16 has three directional lights; the first and the third are
# castshadow="false", the middle one (line 15, dir='-1 1 -1') keeps MuJoCo's default and casts
SHADOW_LIGHT = 1
MODEL_ASSET = os.path.join(os.path.dirname(os.path.abspath(__file__)), "assets", "so100_model.json")
# the keys of a visual-randomisation dict (SO100VecEnv.set_domain_randomization(visual=...), sample_views(ranges))
VISUAL_KEYS = ("camera_pos", "camera_rot_deg", "fovy", "ambient", "headlight", "lights", "light_rot_deg", "colors",
               "per_episode", "seed")


def _torch():
    import torch
    return torch


def load_scene(path=ASSET):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def make_camera(scene, name="top"):
    """so100_camera for one of the scene's cameras (scene_so100.xml:26-29)."""
    if name not in CAMERAS:
        raise ValueError(f"camera {name!r}: one of {CAMERAS}")
    cam = _native.SO100Camera()
    cam.pos[:] = [float(x) for x in scene[f"cam_{name}_pos"]]
    cam.mat[:] = [float(x) for x in scene[f"cam_{name}_mat"].reshape(-1)]
    cam.track = 1 if name in TRACKING else 0
    cam.fovy = float(scene["fovy"])
    cam.znear = ZNEAR
    cam.head_ambient, cam.head_diffuse = (float(x) for x in scene["head"])
    nl = len(scene["light_diffuse"])
    if nl > _native.SO100_MAX_LIGHTS:
        raise ValueError("too many lights")
    cam.nlight = nl
    for i in range(nl):
        cam.light_dir[i][:] = [float(x) for x in scene["light_dir"][i]]
        cam.light_diffuse[i] = float(scene["light_diffuse"][i])
    return cam


def make_mounted_camera(scene, body, pos, mat=None, fovy=None):
    """so100_camera riding on ``body`` (1 Base, 2..7 the arm's links, 8 the cube) under the scene's lights: ``pos`` is in
    the body's frame.  With ``mat`` ([3,3], columns = camera x right, y up, z backward, in the body's frame) it is a rigid
    mount; with mat=None it tracks the ee body from its moving position (mode="targetbody", as left_wrist does).  The
    body rides in the camera's ``frame_body`` attribute, which MultiCameraRenderer reads (a world camera has none)."""
    body = int(body)
    if not 1 <= body < NBODY:
        raise ValueError(f"body {body}: a mounted camera rides on body 1..{NBODY - 1}")
    cam = make_camera(scene, "top")                      # the scene's lights, headlight and znear
    cam.pos[:] = [float(x) for x in pos]
    if mat is None:
        cam.track = 1
        cam.mat[:] = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    else:
        m = np.asarray(mat, dtype=np.float64)
        if m.shape != (3, 3):
            raise ValueError("mat: a [3, 3] rotation in the body's frame")
        cam.track = 0
        cam.mat[:] = [float(x) for x in m.reshape(-1)]
    if fovy is not None:
        cam.fovy = float(fovy)
    if not 0.0 < cam.fovy < 180.0:
        raise ValueError(f"fovy {cam.fovy}: degrees in (0, 180)")
    cam.frame_body = body
    return cam


def camera_by_name(scene, name):
    """so100_camera of a name in CAMERAS (fixed in the world) or MOUNTED_CAMERAS (frame_body set)."""
    if name in _MOUNTED:
        return make_mounted_camera(scene, **_MOUNTED[name])
    if name not in CAMERAS:
        raise ValueError(f"camera {name!r}: one of {CAMERAS + MOUNTED_CAMERAS}")
    return make_camera(scene, name)


def check_camera_names(cameras):
    """The argument check of a ``cameras=`` tuple (no device use): 1..SO100_MAX_CAMS known names.  Returns the tuple."""
    if isinstance(cameras, str):
        raise ValueError("cameras: a tuple of camera names, e.g. ('top', 'left_wrist')")
    names = tuple(cameras)
    if not 1 <= len(names) <= _native.SO100_MAX_CAMS:
        raise ValueError(f"cameras: 1..{_native.SO100_MAX_CAMS} cameras, got {len(names)}")
    for c in names:
        if not isinstance(c, _native.SO100Camera) and c not in CAMERAS + MOUNTED_CAMERAS:
            raise ValueError(f"camera {c!r}: one of {CAMERAS + MOUNTED_CAMERAS}")
    return names


def camera_seed(seed, c):
    """The seed of camera c's view records: the given seed for camera 0 (one camera reproduces CameraRenderer's
    records), else splitmix64(seed + c * 0x9E3779B97F4A7C15 mod 2^64)."""
    x = int(seed) & 0xFFFFFFFFFFFFFFFF
    if c == 0:
        return x
    M = 0xFFFFFFFFFFFFFFFF
    x = (x + c * 0x9E3779B97F4A7C15) & M
    x = (x + 0x9E3779B97F4A7C15) & M
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
    return x ^ (x >> 31)


def material_ids(scene):
    """(ids uint8 [ntri], base float32 [5, 3]): each triangle's material and each material's one base colour, from the
    asset's (body, rgb): body 0 grey 0.2 is the table and grey 0.5 the bin, bodies 1-7 at 1.0 are the arm's light parts
    and at 0.1 its dark parts, body 8 is the cube.  ValueError for a triangle that fits no material and for a material
    with more than one base colour."""
    body = np.asarray(scene["body"])
    rgb = np.asarray(scene["rgb"], dtype=np.float32)
    grey = (rgb[:, 0] == rgb[:, 1]) & (rgb[:, 1] == rgb[:, 2])

    def is_grey(v):
        return grey & (rgb[:, 0] == np.float32(v))
    arm = (body >= 1) & (body <= 7)
    which = [(body == 0) & is_grey(0.2), (body == 0) & is_grey(0.5), arm & is_grey(1.0), arm & is_grey(0.1), body == 8]
    count = np.sum(which, axis=0)
    if np.any(count != 1):
        raise ValueError(f"{int(np.sum(count != 1))} triangles fit no material of {MATERIALS} (or more than one), "
                         f"the first: triangle {int(np.nonzero(count != 1)[0][0])}")
    ids = np.zeros(len(body), dtype=np.uint8)
    base = np.zeros((len(MATERIALS), 3), dtype=np.float32)
    for k, w in enumerate(which):
        ids[w] = k
        cols = np.unique(rgb[w], axis=0)
        if len(cols) > 1:
            raise ValueError(f"material {MATERIALS[k]!r} has {len(cols)} base colours")
        if len(cols):
            base[k] = cols[0]
    return ids, base


def segment_labels(scene):
    """(labels uint8 [ntri], names): each triangle's segmentation class: 0 table and 1 bin (the world body's triangles,
    told apart by material_ids), 2 the Base (body 1), 3-8 the six arm links (bodies 2-7), 9 the cube (body 8); names[k]
    is class k's.  ValueError for a triangle that fits no class."""
    body = np.asarray(scene["body"])
    world = body == 0
    mat, _ = material_ids({"body": body[world], "rgb": np.asarray(scene["rgb"])[world]})     # the world body's alone
    lab = np.full(len(body), SEG_BACKGROUND, dtype=np.uint8)
    lab[np.nonzero(world)[0][mat == MATERIALS.index("table")]] = 0
    lab[np.nonzero(world)[0][mat == MATERIALS.index("bin")]] = 1
    for b in range(1, 9):
        lab[body == b] = b + 1
    bad = np.nonzero(lab == SEG_BACKGROUND)[0]
    if len(bad):
        raise ValueError(f"{len(bad)} triangles fit no segmentation class of {SEG_CLASSES}, the first: triangle "
                         f"{int(bad[0])} (body {int(body[bad[0]])})")
    return lab, SEG_CLASSES


def shadow_casters(scene):
    """uint8 [ntri]: 1 for every triangle that is drawn into the shadow map, the default of ``so100_render_casters``:
    all but the table's 12.  The table only receives: nothing lies under it, and leaving it out removes its
    self-shadowing without a slope bias."""
    mat, _ = material_ids(scene)
    return np.ascontiguousarray(mat != MATERIALS.index("table"), dtype=np.uint8)


def shadow_bounds(scene, model_path=MODEL_ASSET):
    """(center [3], radius): the sphere the default shadow map covers, from the scene's vertices and the model's link
    offsets.  It is the centre and half-diagonal of the box around (a) the bin's vertices, (b) the cube's spawn range
    (constants.SO100_BOX_SPAWN_RANGES) grown by the cube's farthest vertex and (c) the arm's reach, the half-ball above
    z = 0 about the Base's origin whose radius is the chain of link offsets up to Fixed_Jaw plus the farthest vertex of
    the two jaws; the box is clipped to the table's x / y extent, beyond which nothing receives a shadow."""
    with open(model_path) as f:
        body_pos = np.asarray(json.load(f)["body_pos"], dtype=np.float64)
    tri = np.asarray(scene["tri"], dtype=np.float64)
    body = np.asarray(scene["body"])
    mat, _ = material_ids(scene)

    def far(b):
        return float(np.linalg.norm(tri[body == b].reshape(-1, 3), axis=1).max())
    reach = float(np.linalg.norm(body_pos[2:7], axis=1).sum()) + max(far(6), float(np.linalg.norm(body_pos[7])) + far(7))
    lo, hi = body_pos[1] - reach, body_pos[1] + reach
    lo[2] = 0.0
    spawn = np.asarray(SO100_BOX_SPAWN_RANGES, dtype=np.float64)
    binv = tri[mat == MATERIALS.index("bin")].reshape(-1, 3)
    lo = np.minimum(lo, np.minimum(binv.min(axis=0), spawn[:, 0] - far(8)))
    hi = np.maximum(hi, np.maximum(binv.max(axis=0), spawn[:, 1] + far(8)))
    table = tri[mat == MATERIALS.index("table")].reshape(-1, 3)
    lo[:2] = np.maximum(lo[:2], table.min(axis=0)[:2])
    hi[:2] = np.minimum(hi[:2], table.max(axis=0)[:2])
    return 0.5 * (lo + hi), float(0.5 * np.linalg.norm(hi - lo))


SHADOW_KEYS = ("map_size", "bias", "radius", "center", "light")


def make_shadow(scene, map_size=64, bias=0.01, radius=None, center=None, light=SHADOW_LIGHT):
    """so100_shadow for ``so100_render_shadow``: light ``light`` (default SHADOW_LIGHT; -1: nothing casts) casts through
    a map of map_size x map_size texels (a multiple of 8 in 8..64: it lives in LDS) over the sphere (center, radius)
    (default shadow_bounds) with a depth bias in metres.  ValueError for what the library would refuse."""
    c0, r0 = shadow_bounds(scene)
    center = c0 if center is None else np.asarray(center, dtype=np.float64).reshape(-1)
    radius = r0 if radius is None else float(radius)
    map_size, light, bias = int(map_size), int(light), float(bias)
    if map_size < 8 or map_size > _native.SO100_SHADOW_MAP_MAX or map_size % 8:
        raise ValueError(f"map_size {map_size}: a multiple of 8 in 8..{_native.SO100_SHADOW_MAP_MAX} (the shadow map "
                         f"lives in LDS)")
    if not -1 <= light < len(scene["light_diffuse"]):
        raise ValueError(f"light {light}: -1 (nothing casts) or 0..{len(scene['light_diffuse']) - 1}")
    if not (np.isfinite(radius) and radius > 0.0):
        raise ValueError(f"radius {radius!r}: finite and > 0")
    if not (np.isfinite(bias) and bias >= 0.0):
        raise ValueError(f"bias {bias!r}: finite and >= 0")
    if center.shape != (3,) or not np.all(np.isfinite(center)):
        raise ValueError("center: three finite numbers")
    return _native.SO100Shadow(light=light, map_size=map_size, center=center, radius=radius, bias=bias)


def shadow_options(scene, shadows):
    """The ``shadows=`` argument of the renderers and envs (no device use): False / None -> None; True -> make_shadow's
    defaults; a dict with keys of SHADOW_KEYS -> make_shadow(**dict).  ValueError for anything else and unknown keys."""
    if shadows is None or shadows is False:
        return None
    if shadows is True:
        shadows = {}
    if not isinstance(shadows, dict):
        raise ValueError(f"shadows: True, False or a dict with keys of {SHADOW_KEYS}")
    unknown = set(shadows) - set(SHADOW_KEYS)
    if unknown:
        raise ValueError(f"shadows: unknown keys {sorted(unknown)}; known: {SHADOW_KEYS}")
    return make_shadow(scene, **shadows)


# the default sample patterns of so100_render_msaa, offsets from the pixel centre (every number exact in float32): the
# rotated grid for 4 samples, the diagonal pair for 2
AA_PATTERNS = {1: ((0.0, 0.0),),
               2: ((-0.25, -0.25), (0.25, 0.25)),
               4: ((-0.125, -0.375), (0.375, -0.125), (-0.375, 0.125), (0.125, 0.375))}
AA_KEYS = ("samples", "offsets")


def make_antialias(samples=4, offsets=None):
    """so100_msaa for ``so100_render_msaa``: ``samples`` (1, 2 or 4) coverage samples per pixel at ``offsets`` ([samples]
    pairs (x, y) from the pixel centre, each inside (-0.5, 0.5); default AA_PATTERNS[samples]).  ValueError for what
    the library would refuse."""
    if isinstance(samples, bool) or not isinstance(samples, (int, np.integer)) or int(samples) not in AA_PATTERNS:
        raise ValueError(f"samples {samples!r}: 1, 2 or 4")
    samples = int(samples)
    off = np.asarray(AA_PATTERNS[samples] if offsets is None else offsets, dtype=np.float64)
    if off.shape != (samples, 2):
        raise ValueError(f"offsets: {samples} pairs (x, y), got shape {off.shape}")
    if not np.all(np.isfinite(off)) or not np.all(np.abs(off.astype(np.float32)) < 0.5):
        raise ValueError("offsets: finite numbers inside (-0.5, 0.5)")
    return _native.SO100Msaa(samples, off.tolist())


def antialias_options(value):
    """The ``antialias=`` argument of the renderers and envs (no device use): False / None -> None; True -> 4 samples in
    the default pattern; 2 or 4 -> that many in their default pattern; a dict with keys of AA_KEYS ->
    make_antialias(**dict).  ValueError for anything else and unknown keys."""
    if value is None or value is False:
        return None
    if value is True:
        return make_antialias(4)
    if isinstance(value, (int, np.integer)):
        if int(value) not in (2, 4):
            raise ValueError(f"antialias: True, False, 2, 4 or a dict with keys of {AA_KEYS}, got {value!r}")
        return make_antialias(int(value))
    if not isinstance(value, dict):
        raise ValueError(f"antialias: True, False, 2, 4 or a dict with keys of {AA_KEYS}, got {value!r}")
    unknown = set(value) - set(AA_KEYS)
    if unknown:
        raise ValueError(f"antialias: unknown keys {sorted(unknown)}; known: {AA_KEYS}")
    return make_antialias(**value)


def pack_rgb8(rgb):
    """float32 [..., 3] in [0, 1] -> packed RGB8 as so100_render_mesh packs tri_rgb (float32 x * 255 + 0.5, truncated)"""
    x = np.clip(np.asarray(rgb, dtype=np.float32), np.float32(0), np.float32(1))
    q = (x * np.float32(255) + np.float32(0.5)).astype(np.uint32)
    return q[..., 0] | (q[..., 1] << 8) | (q[..., 2] << 16)


def _pair(v, what):
    lo, hi = (float(x) for x in v)
    if not 0.0 <= lo <= hi:
        raise ValueError(f"{what}: a scale range (lo, hi) with 0 <= lo <= hi, got {v!r}")
    return lo, hi


def view_ranges(ranges, seed):
    """so100_view_dr from a visual-randomisation dict (keys VISUAL_KEYS; a missing key leaves that part at its base):
    camera_pos: half-width in metres; camera_rot_deg, light_rot_deg: half-widths in degrees of a rotation vector's
    components; fovy, ambient, headlight: (lo, hi) scales; lights: one (lo, hi) for every directional light or a list
    of one per light; colors: one (lo, hi) or a dict by material name (MATERIALS)."""
    unknown = set(ranges) - set(VISUAL_KEYS)
    if unknown:
        raise ValueError(f"visual randomisation: unknown keys {sorted(unknown)}; known: {VISUAL_KEYS}")
    dr = _native.SO100ViewDR(seed)
    for key, field in (("camera_pos", "cam_pos"), ("camera_rot_deg", "cam_rot"), ("light_rot_deg", "light_rot")):
        hw = float(ranges.get(key, 0.0))
        if not hw >= 0.0:
            raise ValueError(f"{key}: a half-width >= 0, got {hw!r}")
        setattr(dr, field, float(np.radians(hw)) if key.endswith("_deg") else hw)
    for key in ("fovy", "ambient", "headlight"):
        if key in ranges:
            getattr(dr, key)[:] = _pair(ranges[key], key)
    if "lights" in ranges:
        li = ranges["lights"]
        per = [li] * _native.SO100_MAX_LIGHTS if np.ndim(li) == 1 else list(li)
        if len(per) > _native.SO100_MAX_LIGHTS:
            raise ValueError("lights: more ranges than SO100_MAX_LIGHTS")
        for k, v in enumerate(per):
            dr.light[k][:] = _pair(v, "lights")
    if "colors" in ranges:
        co = ranges["colors"]
        if isinstance(co, dict):
            bad = set(co) - set(MATERIALS)
            if bad:
                raise ValueError(f"colors: unknown materials {sorted(bad)}; known: {MATERIALS}")
            co = {MATERIALS.index(k): v for k, v in co.items()}
        else:
            co = {k: co for k in range(len(MATERIALS))}
        for k, v in co.items():
            dr.color[k][:] = _pair(v, "colors")
    return dr


def _upload_casters(venv, scene, shadows):
    """The caster bytes belong to the mesh (a new mesh drops them): uploaded with it by a renderer with shadows, read
    only by so100_render_shadow"""
    if shadows is not None:
        cast = shadow_casters(scene)
        _native.check(venv.lib.so100_render_casters(venv._handle, cast.ctypes.data, len(cast)), "so100_render_casters")


class CameraRenderer:
    """Renders every env of ``venv`` (an SO100VecEnv) from one camera into a persistent uint8 tensor.

    channels_first: ``pixels`` (and every ``out``) is [N,3,H,W], the layout SB3's image policies take, written by
    the render kernel itself (C-ABI ``so100_render_to``, chw sink) instead of a transpose afterwards; the default
    [N,H,W,3] is the reference's.

    depth / segmentation: also keep ``depth`` (float32 [N,H,W], metres along the viewing axis, background 0) and / or
    ``segmentation`` (uint8 [N,H,W], segment_labels' classes, background SEG_BACKGROUND), filled by the launch that
    draws ``pixels`` (C-ABI ``so100_render_aux``).  They have no channel axis: channels_first does not touch them.

    shadows: True (make_shadow's defaults) or a dict with keys of SHADOW_KEYS: the scene's shadow-casting light
    (SHADOW_LIGHT) is occluded per pixel by a shadow map each block builds in the render launch (C-ABI
    ``so100_render_shadow`` with K = 1; the [N,H,W,...] tensors are the same memory as [N,1,H,W,...]).  With the default
    False every call is the one of a renderer without the option.  shadow_mask: also keep ``shadow`` (uint8 [N,H,W]:
    1 where the light is occluded, 0 where lit and on the background); needs shadows.

    antialias: True (4 samples, AA_PATTERNS), 2 or 4, or a dict with keys of AA_KEYS: the colour images are drawn with
    that many coverage samples per pixel and resolved inside the launch (C-ABI ``so100_render_msaa`` with K = 1).  With
    depth / segmentation those two tensors come from a second, aux-only ``so100_render_cams`` launch and are bit for bit
    what they are without antialias.  Not together with shadows (ValueError).  With the default False every call is the
    one of a renderer without the option."""

    def __init__(self, venv, width=640, height=480, camera="top", channels_first=False, depth=False,
                 segmentation=False, shadows=False, shadow_mask=False, antialias=False):
        torch = _torch()
        self.venv = venv
        self.width, self.height = int(width), int(height)
        if not (0 < self.width <= 4096 and 0 < self.height and self.width * self.height <= 1 << 22):
            raise ValueError(f"image {self.width}x{self.height}: width <= 4096 and width*height <= 2^22")
        self.antialias = antialias_options(antialias)     # before any device work
        if self.antialias is not None and shadows:
            raise ValueError("antialias with shadows: the two key arrays times the samples do not fit the band in LDS")
        if self.antialias is not None and self.width * self.antialias.samples > 4096:
            raise ValueError(f"antialias: width {self.width} * samples {self.antialias.samples} > 4096")
        scene = load_scene()
        self.shadows = shadow_options(scene, shadows)     # before any device work
        if shadow_mask and self.shadows is None:
            raise ValueError("shadow_mask needs shadows")
        tri = np.ascontiguousarray(scene["tri"], dtype=np.float32)
        body = np.ascontiguousarray(scene["body"], dtype=np.int32)
        rgb = np.ascontiguousarray(scene["rgb"], dtype=np.float32)
        _native.check(venv.lib.so100_render_mesh(venv._handle, tri.ctypes.data, body.ctypes.data, rgb.ctypes.data,
                                                 len(body)), "so100_render_mesh")
        # the material ids belong to the mesh (a new mesh drops them): uploaded with it, read only by render_views
        mat, base = material_ids(scene)
        _native.check(venv.lib.so100_render_materials(venv._handle, mat.ctypes.data, len(mat)),
                      "so100_render_materials")
        self.base_rgb = np.ascontiguousarray(pack_rgb8(base), dtype=np.uint32)       # [5] packed RGB8 per material
        # so do the labels, read only by render_aux's label sink
        lab, _ = segment_labels(scene)
        _native.check(venv.lib.so100_render_labels(venv._handle, lab.ctypes.data, len(lab)), "so100_render_labels")
        _upload_casters(venv, scene, self.shadows)
        self.views = None                # [N, 40] int32 device tensor of so100_view records, or None: one camera
        self.camera_name = camera
        self.camera = make_camera(scene, camera)
        self.ntri = len(body)
        self.channels_first = bool(channels_first)
        self.image_shape = (3, self.height, self.width) if self.channels_first else (self.height, self.width, 3)
        self.pixels = torch.zeros(venv.num_envs, *self.image_shape, dtype=torch.uint8, device=venv.device)
        self.depth = torch.zeros(venv.num_envs, self.height, self.width, dtype=torch.float32,
                                 device=venv.device) if depth else None
        self.segmentation = torch.full((venv.num_envs, self.height, self.width), SEG_BACKGROUND, dtype=torch.uint8,
                                       device=venv.device) if segmentation else None
        self.shadow = torch.zeros(venv.num_envs, self.height, self.width, dtype=torch.uint8,
                                  device=venv.device) if shadow_mask else None

    def identity_views(self):
        """Set ``views`` to the base view in every env (the renderer's camera, the scene's lights and colours): the
        images are then bit for bit those without views.  Returns the tensor."""
        return self.sample_views({}, 0)

    def sample_views(self, ranges, seed, episode=None, mask=None):
        """Draw the view records of the envs in mask (default all; the others keep theirs) on the device (C-ABI
        so100_views_sample): ranges is a visual-randomisation dict (view_ranges), episode an [N] int32 device tensor
        mixed into every draw (default 0).  A record is a pure function of (seed, global env id, episode).  Allocates
        ``views`` (zeroed) on first use and returns it."""
        torch = _torch()
        v = self.venv
        dr = view_ranges(ranges, seed)
        if episode is not None and (episode.shape != (v.num_envs,) or episode.dtype != torch.int32 or
                                    episode.device != v.device or not episode.is_contiguous()):
            raise ValueError("episode must be a contiguous int32 [N] tensor on the env's device")
        m = None
        if mask is not None:
            if mask.shape != (v.num_envs,) or mask.device != v.device:
                raise ValueError("mask must be an [N] tensor on the env's device")
            m = mask.to(torch.uint8).contiguous()
            self._view_mask_ref = m               # keep alive until the launch has run
        if self.views is None:
            self.views = torch.zeros(v.num_envs, _native.VIEW_WORDS, dtype=torch.int32, device=v.device)
        _native.check(v.lib.so100_views_sample(v._handle, ctypes.byref(dr), ctypes.byref(self.camera),
                                               self.base_rgb.ctypes.data, _native.ptr(episode), _native.ptr(m),
                                               _native.ptr(self.views), v._stream()), "so100_views_sample")
        return self.views

    def render(self, qpos=None, out=None, mask=None, flat=None, views=None, depth=None, segmentation=None, shadow=None):
        """Enqueue the render of qpos (default: the env's state) into out (default self.pixels); mask: [N]
        bool/uint8 device tensor of the envs to draw (the others keep their previous image and flat row).

        flat: a contiguous float32 [N, P] device tensor with P >= 3HW, filled by the same launch: floats [0, 3HW)
        of row i are env i's [H,W,3] bytes / 255 (numpy's float32 division, the reference's env.py:267-270),
        whatever the renderer's own layout; the floats beyond 3HW are left as they are.

        views: an [N, 40] int32 device tensor of so100_view records (default ``self.views``); when there is one, env i
        is drawn from record i (C-ABI so100_render_views), otherwise the calls are those of a renderer without
        views.

        depth, segmentation: contiguous [N, H, W] device tensors, float32 and uint8 (defaults ``self.depth`` and
        ``self.segmentation``); when there is either, the launch is so100_render_aux and fills them with the image,
        otherwise every call is the one of a renderer without them.

        shadow: a contiguous uint8 [N, H, W] device tensor (default ``self.shadow``) for the shadow mask; only a
        renderer with ``shadows`` takes one.  Such a renderer makes every call through so100_render_shadow.

        A renderer with ``antialias`` draws out and flat through so100_render_msaa and, when there is a depth or
        segmentation tensor, those through a second launch (so100_render_cams without colour sinks)."""
        torch = _torch()
        v = self.venv
        q = v.qpos if qpos is None else qpos
        o = self.pixels if out is None else out
        if q.shape != (v.num_envs, v.qpos.shape[1]) or q.dtype != torch.float32 or not q.is_contiguous():
            raise ValueError("qpos must be a contiguous float32 [N, 13] device tensor")
        if o.shape != (v.num_envs, *self.image_shape) or o.dtype != torch.uint8 or not o.is_contiguous():
            raise ValueError("out must be a contiguous uint8 [N, %s] device tensor" %
                             ("3, H, W" if self.channels_first else "H, W, 3"))
        m = None
        if mask is not None:
            if mask.shape != (v.num_envs,) or mask.device != v.device:
                raise ValueError("mask must be an [N] tensor on the env's device")
            m = mask.to(torch.uint8).contiguous()
            self._mask_ref = m                    # keep alive until the launch has run
        vw = self.views if views is None else views
        if vw is not None and (vw.shape != (v.num_envs, _native.VIEW_WORDS) or vw.element_size() != 4 or
                               not vw.is_contiguous() or vw.device != o.device):
            raise ValueError("views must be a contiguous 4-byte [N, 40] device tensor")
        dp = self.depth if depth is None else depth
        sg = self.segmentation if segmentation is None else segmentation
        for t, dt, what in ((dp, torch.float32, "depth must be a contiguous float32"),
                            (sg, torch.uint8, "segmentation must be a contiguous uint8")):
            if t is not None and (t.shape != (v.num_envs, self.height, self.width) or t.dtype != dt or
                                  not t.is_contiguous() or t.device != o.device):
                raise ValueError(what + " [N, H, W] device tensor")
        sm = self.shadow if shadow is None else shadow
        if sm is not None and (self.shadows is None or sm.shape != (v.num_envs, self.height, self.width) or
                               sm.dtype != torch.uint8 or not sm.is_contiguous() or sm.device != o.device):
            raise ValueError("shadow must be a contiguous uint8 [N, H, W] device tensor, of a renderer with shadows")
        if flat is None and not self.channels_first and vw is None and dp is None and sg is None and \
                self.shadows is None and self.antialias is None:
            _native.check(v.lib.so100_render(v._handle, _native.ptr(q), _native.ptr(m), ctypes.byref(self.camera),
                                             self.width, self.height, _native.ptr(o), v._stream()), "so100_render")
            return o
        pitch = 0
        if flat is not None:
            if flat.dim() != 2 or flat.shape[0] != v.num_envs or flat.shape[1] < 3 * self.width * self.height or \
                    flat.dtype != torch.float32 or not flat.is_contiguous() or flat.device != o.device:
                raise ValueError("flat must be a contiguous float32 [N, P >= 3*H*W] device tensor")
            pitch = flat.shape[1]
        sinks = _native.SO100ImageOut(hwc=None if self.channels_first else _native.ptr(o),
                                      chw=_native.ptr(o) if self.channels_first else None,
                                      flat=_native.ptr(flat), flat_pitch=pitch)
        if self.antialias is not None:
            # K = 1 of the launch over (env, camera).  Depth and labels are pixel-centre quantities: a second, aux-only
            # so100_render_cams launch draws them, bit for bit what they are without antialias
            cams = _native.SO100Cams([self.camera], [0])
            _native.check(v.lib.so100_render_msaa(v._handle, _native.ptr(q), _native.ptr(m), ctypes.byref(cams),
                                                  _native.ptr(vw), self.width, self.height, ctypes.byref(sinks),
                                                  ctypes.byref(self.antialias), v._stream()), "so100_render_msaa")
            if dp is not None or sg is not None:
                aux = _native.SO100AuxOut(depth=_native.ptr(dp), label=_native.ptr(sg))
                _native.check(v.lib.so100_render_cams(v._handle, _native.ptr(q), _native.ptr(m), ctypes.byref(cams),
                                                      _native.ptr(vw), self.width, self.height, None,
                                                      ctypes.byref(aux), v._stream()), "so100_render_cams")
            return o
        if self.shadows is not None:
            # K = 1 of the launch over (env, camera): [N, ...] is [N, 1, ...] and [N, 40] records are [1, N, 40]
            aux = _native.SO100AuxOut(depth=_native.ptr(dp), label=_native.ptr(sg))
            cams = _native.SO100Cams([self.camera], [0])
            self.shadows.shadow_out = _native.ptr(sm)
            _native.check(v.lib.so100_render_shadow(v._handle, _native.ptr(q), _native.ptr(m), ctypes.byref(cams),
                                                    _native.ptr(vw), self.width, self.height, ctypes.byref(sinks),
                                                    ctypes.byref(aux), ctypes.byref(self.shadows), v._stream()),
                          "so100_render_shadow")
            return o
        if dp is not None or sg is not None:
            aux = _native.SO100AuxOut(depth=_native.ptr(dp), label=_native.ptr(sg))
            _native.check(v.lib.so100_render_aux(v._handle, _native.ptr(q), _native.ptr(m), ctypes.byref(self.camera),
                                                 _native.ptr(vw), self.width, self.height, ctypes.byref(sinks),
                                                 ctypes.byref(aux), v._stream()), "so100_render_aux")
            return o
        if vw is not None:
            _native.check(v.lib.so100_render_views(v._handle, _native.ptr(q), _native.ptr(m), ctypes.byref(self.camera),
                                                   _native.ptr(vw), self.width, self.height, ctypes.byref(sinks),
                                                   v._stream()), "so100_render_views")
            return o
        _native.check(v.lib.so100_render_to(v._handle, _native.ptr(q), _native.ptr(m), ctypes.byref(self.camera),
                                            self.width, self.height, ctypes.byref(sinks), v._stream()),
                      "so100_render_to")
        return o


class MultiCameraRenderer:
    """Renders every env of ``venv`` from K <= 4 cameras with one HIP launch per call (C-ABI ``so100_render_cams``, grid
    (env, camera)) into persistent tensors with the camera axis after the env's.

    cameras: names of CAMERAS / MOUNTED_CAMERAS, or so100_camera structs (make_camera, make_mounted_camera).
    ``pixels`` is uint8 [N,K,H,W,3], with channels_first [N,K,3,H,W] (its free reshape [N,3K,H,W] is the channel-stacked
    image a CNN takes); ``depth`` float32 and ``segmentation`` uint8 are [N,K,H,W]; ``views`` is [K,N,40], camera-major,
    so that each camera's records are the contiguous [N,40] array so100_views_sample fills.  A mounted camera's records
    hold pos (and mat) in its body's frame: camera jitter is then a mount tolerance.

    shadows, shadow_mask: as CameraRenderer's; the launch is then ``so100_render_shadow`` (each (env, camera) block builds
    the map for itself) and ``shadow`` is uint8 [N,K,H,W].

    antialias: as CameraRenderer's: the colour images come from one ``so100_render_msaa`` launch, depth and
    segmentation (if kept) from a second, aux-only ``so100_render_cams`` launch; not together with shadows."""

    def __init__(self, venv, width=640, height=480, cameras=("top", "angle", "front_close"), channels_first=False,
                 depth=False, segmentation=False, shadows=False, shadow_mask=False, antialias=False):
        torch = _torch()
        self.venv = venv
        self.width, self.height = int(width), int(height)
        names = check_camera_names(cameras)
        K = self.ncam = len(names)
        if not (0 < self.width <= 4096 and 0 < self.height and self.width * self.height * K <= 1 << 22):
            raise ValueError(f"image {self.width}x{self.height} x {K} cameras: width <= 4096 and "
                             f"width*height*cameras <= 2^22")
        self.antialias = antialias_options(antialias)     # before any device work
        if self.antialias is not None and shadows:
            raise ValueError("antialias with shadows: the two key arrays times the samples do not fit the band in LDS")
        if self.antialias is not None and self.width * self.antialias.samples > 4096:
            raise ValueError(f"antialias: width {self.width} * samples {self.antialias.samples} > 4096")
        scene = load_scene()
        self.shadows = shadow_options(scene, shadows)     # before any device work
        if shadow_mask and self.shadows is None:
            raise ValueError("shadow_mask needs shadows")
        tri = np.ascontiguousarray(scene["tri"], dtype=np.float32)
        body = np.ascontiguousarray(scene["body"], dtype=np.int32)
        rgb = np.ascontiguousarray(scene["rgb"], dtype=np.float32)
        _native.check(venv.lib.so100_render_mesh(venv._handle, tri.ctypes.data, body.ctypes.data, rgb.ctypes.data,
                                                 len(body)), "so100_render_mesh")
        mat, base = material_ids(scene)
        _native.check(venv.lib.so100_render_materials(venv._handle, mat.ctypes.data, len(mat)),
                      "so100_render_materials")
        self.base_rgb = np.ascontiguousarray(pack_rgb8(base), dtype=np.uint32)
        lab, _ = segment_labels(scene)
        _native.check(venv.lib.so100_render_labels(venv._handle, lab.ctypes.data, len(lab)), "so100_render_labels")
        _upload_casters(venv, scene, self.shadows)
        self.camera_names = tuple(c if isinstance(c, str) else f"camera{k}" for k, c in enumerate(names))
        self.cameras = [camera_by_name(scene, c) if isinstance(c, str) else c for c in names]
        self.frame_body = tuple(int(getattr(c, "frame_body", 0)) for c in self.cameras)
        self.cams = _native.SO100Cams(self.cameras, self.frame_body)
        self.views = None                # [K, N, 40] int32 device tensor of so100_view records, or None
        self.ntri = len(body)
        self.channels_first = bool(channels_first)
        self.image_shape = (K, 3, self.height, self.width) if self.channels_first else (K, self.height, self.width, 3)
        n, d = venv.num_envs, venv.device
        self.pixels = torch.zeros(n, *self.image_shape, dtype=torch.uint8, device=d)
        self.depth = torch.zeros(n, K, self.height, self.width, dtype=torch.float32, device=d) if depth else None
        self.segmentation = torch.full((n, K, self.height, self.width), SEG_BACKGROUND, dtype=torch.uint8,
                                       device=d) if segmentation else None
        self.shadow = torch.zeros(n, K, self.height, self.width, dtype=torch.uint8, device=d) if shadow_mask else None

    def identity_views(self):
        """Set ``views`` to each camera's base view in every env: the images are then bit for bit those without
        views.  Returns the tensor."""
        return self.sample_views({}, 0)

    def sample_views(self, ranges, seed, episode=None, mask=None):
        """CameraRenderer.sample_views per camera: one so100_views_sample call on camera c's slice ``views[c]`` with
        camera c as the base and the seed camera_seed(seed, c), so a record is a pure function of (seed, camera, global
        env id, episode) and one camera reproduces CameraRenderer's records.  Allocates ``views`` on first use."""
        torch = _torch()
        v = self.venv
        if episode is not None and (episode.shape != (v.num_envs,) or episode.dtype != torch.int32 or
                                    episode.device != v.device or not episode.is_contiguous()):
            raise ValueError("episode must be a contiguous int32 [N] tensor on the env's device")
        m = None
        if mask is not None:
            if mask.shape != (v.num_envs,) or mask.device != v.device:
                raise ValueError("mask must be an [N] tensor on the env's device")
            m = mask.to(torch.uint8).contiguous()
            self._view_mask_ref = m               # keep alive until the launches have run
        if self.views is None:
            self.views = torch.zeros(self.ncam, v.num_envs, _native.VIEW_WORDS, dtype=torch.int32, device=v.device)
        for c in range(self.ncam):
            dr = view_ranges(ranges, camera_seed(seed, c))
            _native.check(v.lib.so100_views_sample(v._handle, ctypes.byref(dr), ctypes.byref(self.cameras[c]),
                                                   self.base_rgb.ctypes.data, _native.ptr(episode), _native.ptr(m),
                                                   _native.ptr(self.views[c]), v._stream()), "so100_views_sample")
        return self.views

    def render(self, qpos=None, out=None, mask=None, flat=None, views=None, depth=None, segmentation=None, shadow=None):
        """Enqueue the one launch that draws qpos (default: the env's state) from every camera into out (default
        ``self.pixels``).  mask: [N] envs to draw, in all their cameras (the others keep every image and flat row).
        flat: contiguous float32 [N, P >= K*3HW]: floats [c*3HW, (c+1)*3HW) of row i are camera c's [H,W,3] bytes / 255.
        views: [K, N, 40] records (default ``self.views``).  depth, segmentation: [N, K, H, W] (defaults the
        renderer's own).  shadow: uint8 [N, K, H, W] for the shadow mask (default ``self.shadow``), of a renderer with
        ``shadows`` only; such a renderer's launch is so100_render_shadow.  A renderer with ``antialias`` draws out and
        flat through so100_render_msaa and depth / segmentation, if any, through a second launch."""
        torch = _torch()
        v = self.venv
        K, H, W = self.ncam, self.height, self.width
        q = v.qpos if qpos is None else qpos
        o = self.pixels if out is None else out
        if q.shape != (v.num_envs, v.qpos.shape[1]) or q.dtype != torch.float32 or not q.is_contiguous():
            raise ValueError("qpos must be a contiguous float32 [N, 13] device tensor")
        if o.shape != (v.num_envs, *self.image_shape) or o.dtype != torch.uint8 or not o.is_contiguous():
            raise ValueError("out must be a contiguous uint8 [N, K, %s] device tensor" %
                             ("3, H, W" if self.channels_first else "H, W, 3"))
        m = None
        if mask is not None:
            if mask.shape != (v.num_envs,) or mask.device != v.device:
                raise ValueError("mask must be an [N] tensor on the env's device")
            m = mask.to(torch.uint8).contiguous()
            self._mask_ref = m                    # keep alive until the launch has run
        vw = self.views if views is None else views
        if vw is not None and (vw.shape != (K, v.num_envs, _native.VIEW_WORDS) or vw.element_size() != 4 or
                               not vw.is_contiguous() or vw.device != o.device):
            raise ValueError("views must be a contiguous 4-byte [K, N, 40] device tensor")
        dp = self.depth if depth is None else depth
        sg = self.segmentation if segmentation is None else segmentation
        for t, dt, what in ((dp, torch.float32, "depth must be a contiguous float32"),
                            (sg, torch.uint8, "segmentation must be a contiguous uint8")):
            if t is not None and (t.shape != (v.num_envs, K, H, W) or t.dtype != dt or not t.is_contiguous() or
                                  t.device != o.device):
                raise ValueError(what + " [N, K, H, W] device tensor")
        sm = self.shadow if shadow is None else shadow
        if sm is not None and (self.shadows is None or sm.shape != (v.num_envs, K, H, W) or sm.dtype != torch.uint8 or
                               not sm.is_contiguous() or sm.device != o.device):
            raise ValueError("shadow must be a contiguous uint8 [N, K, H, W] device tensor, of a renderer with shadows")
        pitch = 0
        if flat is not None:
            if flat.dim() != 2 or flat.shape[0] != v.num_envs or flat.shape[1] < K * 3 * W * H or \
                    flat.dtype != torch.float32 or not flat.is_contiguous() or flat.device != o.device:
                raise ValueError("flat must be a contiguous float32 [N, P >= K*3*H*W] device tensor")
            pitch = flat.shape[1]
        sinks = _native.SO100ImageOut(hwc=None if self.channels_first else _native.ptr(o),
                                      chw=_native.ptr(o) if self.channels_first else None,
                                      flat=_native.ptr(flat), flat_pitch=pitch)
        aux = _native.SO100AuxOut(depth=_native.ptr(dp), label=_native.ptr(sg))
        if self.antialias is not None:
            # depth and labels are pixel-centre quantities: a second, aux-only so100_render_cams launch draws them
            _native.check(v.lib.so100_render_msaa(v._handle, _native.ptr(q), _native.ptr(m), ctypes.byref(self.cams),
                                                  _native.ptr(vw), W, H, ctypes.byref(sinks),
                                                  ctypes.byref(self.antialias), v._stream()), "so100_render_msaa")
            if dp is not None or sg is not None:
                _native.check(v.lib.so100_render_cams(v._handle, _native.ptr(q), _native.ptr(m), ctypes.byref(self.cams),
                                                      _native.ptr(vw), W, H, None, ctypes.byref(aux), v._stream()),
                              "so100_render_cams")
            return o
        if self.shadows is not None:
            self.shadows.shadow_out = _native.ptr(sm)
            _native.check(v.lib.so100_render_shadow(v._handle, _native.ptr(q), _native.ptr(m), ctypes.byref(self.cams),
                                                    _native.ptr(vw), W, H, ctypes.byref(sinks), ctypes.byref(aux),
                                                    ctypes.byref(self.shadows), v._stream()), "so100_render_shadow")
            return o
        _native.check(v.lib.so100_render_cams(v._handle, _native.ptr(q), _native.ptr(m), ctypes.byref(self.cams),
                                              _native.ptr(vw), W, H, ctypes.byref(sinks), ctypes.byref(aux),
                                              v._stream()), "so100_render_cams")
        return o
