"""numpy restatement of csrc/so100_render_msaa.hip's rules (TEST INFRASTRUCTURE ONLY): render_aux_ref.render's colour
path with a sample axis and the resolve.

A launch has S samples per pixel at offsets (ox_s, oy_s) from the pixel centre; sample s of pixel (x, y) is the point
(x + 0.5 + ox_s, y + 0.5 + oy_s), added in that order.  Coverage (inclusive edge functions, the |area| > 1e-12 reject),
the perspective-correct depth (izp > 0) and the key depth bits << 32 | packed RGB under a minimum are render_aux_ref's
rules at that point; a triangle is shaded once and every sample takes its flat colour.  The triangle's box of pixels is
[floor(min - 0.5 - max_s o_s), ceil(max - 0.5 - min_s o_s)] clipped to the image.  The resolved byte of a pixel and
channel is (sum over s of the samples' bytes + S // 2) // S, an empty sample counting 0.  ``dtype`` sets the arithmetic,
as in render_aux_ref.  Also the sample patterns and the box mean the tests share.
"""
import numpy as np

import render_aux_ref as A
import render_ref

EMPTY = A.EMPTY
ROTATED4 = ((-0.125, -0.375), (0.375, -0.125), (-0.375, 0.125), (0.125, 0.375))
DIAG2 = ((-0.25, -0.25), (0.25, 0.25))
# the ordered grid in the order of the 2 x 2 block of a 2W x 2H image: (left, top), (right, top), (left, bottom), ...
ORDERED4 = ((-0.25, -0.25), (0.25, -0.25), (-0.25, 0.25), (0.25, 0.25))
CENTRE1 = ((0.0, 0.0),)


def box_mean(img, f=2):
    """uint8 [f H, f W, 3] -> uint8 [H, W, 3]: the round-half-up mean of every f x f block, in integers."""
    h, w = img.shape[0] // f, img.shape[1] // f
    s = img.astype(np.uint32).reshape(h, f, w, f, 3).sum(axis=(1, 3))
    return ((s + (f * f) // 2) // (f * f)).astype(np.uint8)


def resolve(samples):
    """uint8 [S, H, W, 3] (an empty sample 0) -> uint8 [H, W, 3]: (sum + S // 2) // S"""
    S = samples.shape[0]
    return ((samples.astype(np.uint32).sum(axis=0) + S // 2) // S).astype(np.uint8)


def raster(sx, sy, iz, ok, col, width, height, offsets, dt, winner=False):
    """The sample keys of set-up triangles: sx, sy, iz [T, 3] screen vertices and inverse depths, ok [T] (every vertex
    beyond znear), col [T] packed RGB.  Returns uint8 [S, H, W, 3], the colour every sample holds (empty: 0), and with
    winner=True also int32 [S, H, W]: the index of the triangle whose key the sample holds (the first of equal keys),
    -1 for an empty sample."""
    off = np.asarray(offsets, np.float64).astype(dt)
    S = len(off)
    key = np.full((S, height, width), EMPTY, np.uint64)
    win = np.full((S, height, width), -1, np.int32)
    half = dt(0.5)
    oxlo, oxhi, oylo, oyhi = off[:, 0].min(), off[:, 0].max(), off[:, 1].min(), off[:, 1].max()
    for t in np.nonzero(ok)[0]:
        x, y, z = sx[t], sy[t], iz[t]
        area = (x[1] - x[0]) * (y[2] - y[0]) - (x[2] - x[0]) * (y[1] - y[0])
        if not abs(area) > 1e-12:
            continue
        bx0 = max(0, int(np.floor(x.min() - half - oxhi)))
        bx1 = min(width - 1, int(np.ceil(x.max() - half - oxlo)))
        by0 = max(0, int(np.floor(y.min() - half - oyhi)))
        by1 = min(height - 1, int(np.ceil(y.max() - half - oylo)))
        if bx0 > bx1 or by0 > by1:
            continue
        cx, cy = np.meshgrid(np.arange(bx0, bx1 + 1).astype(dt) + half, np.arange(by0, by1 + 1).astype(dt) + half)
        sg = dt(1.0) if area > 0 else dt(-1.0)
        for s in range(S):
            px, py = cx + off[s, 0], cy + off[s, 1]
            w0 = (x[2] - x[1]) * (py - y[1]) - (y[2] - y[1]) * (px - x[1])
            w1 = (x[0] - x[2]) * (py - y[2]) - (y[0] - y[2]) * (px - x[2])
            w2 = (x[1] - x[0]) * (py - y[0]) - (y[1] - y[0]) * (px - x[0])
            inside = (w0 * sg >= 0) & (w1 * sg >= 0) & (w2 * sg >= 0)
            izp = (w0 * z[0] + w1 * z[1] + w2 * z[2]) / area
            inside &= izp > 0
            dep = (dt(1.0) / np.where(inside, izp, dt(1.0))).astype(np.float32)
            k = (dep.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(col[t])
            sub = key[s, by0:by1 + 1, bx0:bx1 + 1]
            np.copyto(win[s, by0:by1 + 1, bx0:bx1 + 1], np.int32(t), where=inside & (k < sub))
            np.copyto(sub, np.minimum(sub, k), where=inside)
    rgb = np.where(key == EMPTY, np.uint64(0), key & np.uint64(0xFFFFFF)).astype(np.uint32)
    smp = np.stack([(rgb >> (8 * k)) & 0xFF for k in range(3)], axis=-1).astype(np.uint8)
    return (smp, win) if winner else smp


def render(scene_tri, scene_body, scene_rgb, frames, cam, width, height, offsets, target=None, dtype=np.float64,
           winner=False):
    """render_aux_ref.render's arguments without the labels, plus offsets [S][2].  Returns (rgb uint8 [H,W,3] resolved,
    samples uint8 [S,H,W,3]) and with winner=True a third, int32 [S,H,W]: each sample's winning triangle (-1: empty)."""
    dt = np.dtype(dtype).type
    cam = dict(cam, pos=np.asarray(cam["pos"], dt), mat=np.asarray(cam["mat"], dt), fovy=dt(cam["fovy"]),
               znear=dt(cam["znear"]), head_ambient=dt(cam["head_ambient"]), head_diffuse=dt(cam["head_diffuse"]),
               light_dir=[np.asarray(d, dt) for d in cam["light_dir"]],
               light_diffuse=[dt(c) for c in cam["light_diffuse"]])
    if cam.get("track"):
        cam["mat"] = A._tracking_frame(cam["pos"], np.asarray(target, dt), dt)
    R = np.stack([f[0] for f in frames]).astype(dt)[scene_body]
    P = np.stack([f[1] for f in frames]).astype(dt)[scene_body]
    w = np.einsum("tij,tvj->tvi", R, scene_tri.astype(dt)) + P[:, None, :]
    c = (w - cam["pos"]) @ cam["mat"]
    depth = -c[..., 2]
    th = np.tan(dt(0.5) * np.radians(cam["fovy"]))
    aspect = dt(width) / dt(height)
    ok = np.all(depth > cam["znear"], axis=1)
    iz = dt(1.0) / np.where(depth > 0, depth, dt(1.0))
    sx = (c[..., 0] * iz / (th * aspect) * dt(0.5) + dt(0.5)) * dt(width)
    sy = (dt(0.5) - c[..., 1] * iz / th * dt(0.5)) * dt(height)
    col = A._shade(cam, w, render_ref.pack_rgb(scene_rgb), dt)
    if winner:
        smp, win = raster(sx, sy, iz, ok, col, width, height, offsets, dt, winner=True)
        return resolve(smp), smp, win
    smp = raster(sx, sy, iz, ok, col, width, height, offsets, dt)
    return resolve(smp), smp


_CACHE = {}


def reference(model, oracle, bits, offsets, scale=1):
    """The restatement's resolved images of the first three sets of render_aux_ref.scene_states() at (scale W) x
    (scale H) in float`bits` arithmetic on `oracle`'s frames, computed once per session and shared (read only):
    [(camera, W, H, qpos, [rgb] per env)] with W, H the set's own (unscaled)."""
    k = (bits, tuple(map(tuple, offsets)), scale)
    if k in _CACHE:
        return _CACHE[k]
    from gym_so100 import render as R
    scene = R.load_scene()
    out = []
    for name, w, h, qpos in A.scene_states()[:3]:
        cam = render_ref.camera_dict(R.make_camera(scene, name))
        imgs = []
        for q in qpos:
            fr, ee = A.frames_of(oracle, model, q.astype(np.float64))
            imgs.append(render(scene["tri"], scene["body"], scene["rgb"], fr, cam, scale * w, scale * h, offsets,
                               target=ee, dtype=np.float64 if bits == 64 else np.float32)[0])
        out.append((name, w, h, qpos, imgs))
    _CACHE[k] = out
    return out


_WRIST = {}


def reference_wrist(model, oracle, offsets, count=3):
    """left_wrist at 64x48 (render_cams_ref's camera and states, the first `count`) in float64: [rgb] per state."""
    import render_cams_ref as C
    k = (tuple(map(tuple, offsets)), count)
    if k in _WRIST:
        return _WRIST[k]
    from gym_so100 import render as R
    scene = R.load_scene()
    cam, fb = C.mounted_cameras(R, scene)["left_wrist"]
    out = []
    for q in C.states()[:count]:
        fr, ee = A.frames_of(oracle, model, q.astype(np.float64))
        wc = C.world_camera(render_ref.camera_dict(cam), fb, fr, np.float64)
        out.append(render(scene["tri"], scene["body"], scene["rgb"], fr, wc, C.W, C.H, offsets, target=ee)[0])
    _WRIST[k] = out
    return out
