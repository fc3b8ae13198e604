"""numpy restatement of csrc/so100_render_shadow.hip's rules (TEST INFRASTRUCTURE ONLY), on render_aux_ref.render.

Light frame: d the casting light's normalised direction, u = normalize(z x d) (x if |z x d| < 1e-6), v = d x u.  With
the map's centre c, radius r and size S a world point P has map coordinates a = ((P-c).u / r * 0.5 + 0.5) * S, b likewise
with v, and depth (P-c).d.  The map: every caster triangle rasterised with the camera rasteriser's rules (texel centres
at +0.5, inclusive edge functions, the |area| > 1e-12 reject), depth linear in the edge weights, a texel holds the
smallest float32 depth or is empty.  A pixel with a winning key is shadowed iff the point its centre sees at the key's
float32 depth, P = pos + depth * mat.(xn, yn, -1), falls on a texel inside the map that is not empty and holds a depth
< (P-c).d - bias.  A shadowed pixel takes the colour of the image drawn with the casting light's diffuse 0, every other
pixel, the depth and the labels are render_aux_ref.render's.

``dtype`` sets the arithmetic (float64: the reference the GPU is held to; float32: what the number format alone costs).
Also the lifted-cube state and the tests' shared references.
"""
import numpy as np

import render_aux_ref as A
import render_cams_ref as C
import render_ref

# the largest share of an image's pixels (among those whose label agrees) at which the float32 restatement's mask (on
# oracle32's frames) differs from the float64 one (on oracle64's), over render_aux_ref.SCENE_SETS' 12 images (each set's
# own camera and size, 640x480 included) and the lifted-cube state from `top` at 64x48 and 96x72, default map: measured
# by test_render_shadow_cpu.py (test_float32_floor): 0 differing pixels in all 14 images, whose shadowed shares are
# 0.56 % (angle 37x29) to 3.1 % (the lifted cube).  The GPU's bar is twice this plus 2 pixels per image, so the 2
# pixels are all of it
MASK_F32_FLOOR = 0.0
# the cube lifted to z = 0.15 over the table at the spawn range's middle, identity rotation, arm at its zero pose
LIFTED = np.array([0, 0, 0, 0, 0, 0, -0.05, 0.55, 0.15, 1, 0, 0, 0], np.float32)


def light_frame(direction, dt):
    d = np.asarray(direction, dt)
    d = d / np.sqrt(np.sum(d * d))
    u = np.array([-d[1], d[0], dt(0.0)], dt)                 # z x d
    n = np.sqrt(np.sum(u * u))
    u = u / n if not n < 1e-6 else np.array([1.0, 0.0, 0.0], dt)
    return d, u, np.cross(d, u).astype(dt)


def shadow_map(scene_tri, scene_body, caster, frames, frame, center, radius, S, dtype=np.float64):
    """float32 [S, S] (row b, column a) of the smallest depth per texel, +inf where empty."""
    dt = np.dtype(dtype).type
    d, u, v = frame
    idx = np.nonzero(caster)[0]
    R = np.stack([f[0] for f in frames]).astype(dt)[scene_body[idx]]
    P = np.stack([f[1] for f in frames]).astype(dt)[scene_body[idx]]
    w = np.einsum("tij,tvj->tvi", R, scene_tri[idx].astype(dt)) + P[:, None, :] - np.asarray(center, dt)
    sc = dt(0.5) / dt(radius)
    sx = ((w @ u) * sc + dt(0.5)) * dt(S)
    sy = ((w @ v) * sc + dt(0.5)) * dt(S)
    dz = w @ d
    out = np.full((S, S), np.inf, np.float32)
    half = dt(0.5)
    for t in range(len(idx)):
        x, y, z = sx[t], sy[t], dz[t]
        area = (x[1] - x[0]) * (y[2] - y[0]) - (x[2] - x[0]) * (y[1] - y[0])
        if not abs(area) > 1e-12:
            continue
        bx0, bx1 = max(0, int(np.floor(x.min() - half))), min(S - 1, int(np.ceil(x.max() - half)))
        by0, by1 = max(0, int(np.floor(y.min() - half))), min(S - 1, int(np.ceil(y.max() - half)))
        if bx0 > bx1 or by0 > by1:
            continue
        px, py = np.meshgrid(np.arange(bx0, bx1 + 1).astype(dt) + half, np.arange(by0, by1 + 1).astype(dt) + half)
        w0 = (x[2] - x[1]) * (py - y[1]) - (y[2] - y[1]) * (px - x[1])
        w1 = (x[0] - x[2]) * (py - y[2]) - (y[0] - y[2]) * (px - x[2])
        w2 = (x[1] - x[0]) * (py - y[0]) - (y[1] - y[0]) * (px - x[0])
        sg = dt(1.0) if area > 0 else dt(-1.0)
        inside = (w0 * sg >= 0) & (w1 * sg >= 0) & (w2 * sg >= 0)
        dep = ((w0 * z[0] + w1 * z[1] + w2 * z[2]) * (dt(1.0) / area)).astype(np.float32)
        sub = out[by0:by1 + 1, bx0:bx1 + 1]
        np.copyto(sub, np.minimum(sub, dep), where=inside)
    return out


def shadow_mask(depth, lab, cam, width, height, smap, frame, center, radius, bias, target=None, dtype=np.float64):
    """bool [H, W]: the shadow test of every pixel with a winning key (lab != 255) at its float32 depth."""
    dt = np.dtype(dtype).type
    d, u, v = frame
    S = smap.shape[0]
    pos, mat = np.asarray(cam["pos"], dt), np.asarray(cam["mat"], dt)
    if cam.get("track"):
        mat = A._tracking_frame(pos, np.asarray(target, dt), dt)
    th = np.tan(dt(0.5) * np.radians(dt(cam["fovy"])))
    aspect = dt(width) / dt(height)
    x, y = np.meshgrid(np.arange(width).astype(dt), np.arange(height).astype(dt))
    xn = ((x + dt(0.5)) / dt(width) - dt(0.5)) * dt(2.0) * th * aspect
    yn = (dt(0.5) - (y + dt(0.5)) / dt(height)) * dt(2.0) * th
    ray = xn[..., None] * mat[:, 0] + yn[..., None] * mat[:, 1] - mat[:, 2]
    p = pos + depth.astype(dt)[..., None] * ray - np.asarray(center, dt)
    sc = dt(0.5) / dt(radius)
    fa = np.floor(((p @ u) * sc + dt(0.5)) * dt(S))
    fb = np.floor(((p @ v) * sc + dt(0.5)) * dt(S))
    inside = (fa >= 0) & (fa < S) & (fb >= 0) & (fb < S) & (lab != A.BACKGROUND)
    ia, ib = np.where(inside, fa, 0).astype(np.int64), np.where(inside, fb, 0).astype(np.int64)
    tex = smap[ib, ia]
    return inside & np.isfinite(tex) & (tex.astype(dt) < (p @ d) - dt(bias))


def render(scene_tri, scene_body, scene_rgb, label, caster, frames, cam, width, height, shadow, target=None,
           dtype=np.float64):
    """cam: render_ref.camera_dict's dict (a world camera); shadow: dict(light, map_size, center, radius, bias), light
    -1 = nothing casts.  Returns (rgb uint8 [H,W,3], depth float32 [H,W], label uint8 [H,W], mask bool [H,W])."""
    full, dep, lab = A.render(scene_tri, scene_body, scene_rgb, label, frames, cam, width, height, target=target,
                              dtype=dtype)
    s = int(shadow["light"])
    if s < 0:
        return full, dep, lab, np.zeros((height, width), bool)
    diffuse = list(cam["light_diffuse"])
    diffuse[s] = 0.0
    dark, dep2, _ = A.render(scene_tri, scene_body, scene_rgb, label, frames, dict(cam, light_diffuse=diffuse), width,
                             height, target=target, dtype=dtype)
    assert np.array_equal(dep.view(np.uint32), dep2.view(np.uint32))
    dt = np.dtype(dtype).type
    frame = light_frame(cam["light_dir"][s], dt)
    smap = shadow_map(scene_tri, scene_body, caster, frames, frame, shadow["center"], shadow["radius"],
                      int(shadow["map_size"]), dtype)
    mask = shadow_mask(dep, lab, cam, width, height, smap, frame, shadow["center"], shadow["radius"], shadow["bias"],
                       target=target, dtype=dtype)
    return np.where(mask[..., None], dark, full), dep, lab, mask


def shadow_dict(s):
    """so100_shadow ctypes struct -> the dict render() takes (the struct's float32 values)"""
    return dict(light=int(s.light), map_size=int(s.map_size), center=np.array(s.center[:], np.float64),
                radius=float(s.radius), bias=float(s.bias))


def states():
    """float32 [13, 13]: render_aux_ref.scene_states()'s 12 states, then the lifted-cube state."""
    return np.concatenate([C.states(), LIFTED[None]]).astype(np.float32)


_CACHE = {}


def reference(model, oracle, bits, camera, width, height, map_size=64):
    """[(rgb, depth, label, mask)] per state of states(): `camera` (a name of render.CAMERAS / MOUNTED_CAMERAS) at
    width x height with make_shadow's defaults at map_size, in float`bits` arithmetic on `oracle`'s frames; computed once
    per session and shared (read only)."""
    key = (bits, camera, width, height, map_size)
    if key in _CACHE:
        return _CACHE[key]
    from gym_so100 import render as R
    scene = R.load_scene()
    lab, _ = R.segment_labels(scene)
    cast = R.shadow_casters(scene)
    sh = shadow_dict(R.make_shadow(scene, map_size=map_size))
    cam = R.camera_by_name(scene, camera)
    fb = int(getattr(cam, "frame_body", 0))
    dtype = np.float64 if bits == 64 else np.float32
    out = []
    for q in states():
        fr, ee = A.frames_of(oracle, model, q.astype(np.float64))
        wc = C.world_camera(render_ref.camera_dict(cam), fb, fr, dtype)
        out.append(render(scene["tri"], scene["body"], scene["rgb"], lab, cast, fr, wc, width, height, sh, target=ee,
                          dtype=dtype))
    _CACHE[key] = out
    return out
