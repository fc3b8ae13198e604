"""numpy restatement of csrc/so100_render_aux.hip's rules (TEST INFRASTRUCTURE ONLY): render_ref.render's rasterisation
with the key of the aux kernel, depth bits << 32 | RGB8 << 8 | label, returning the colour, depth and label images.

The rules are render_ref's: pixel centres inside a triangle by its three edge functions (edges included),
perspective-correct depth, the nearest depth wins; equal depths take the smaller packed RGB and, new here, equal colours
the smaller label.  Depth is the float32 that was compared (1 / izp: metres along the camera's viewing axis), 0 on the
background; the background's label is 255.  ``dtype`` sets the arithmetic: float64 (the reference the GPU is held to;
its RGB equals render_ref.render's exactly) or float32 (numpy's float32, which measures what the number format alone
costs).  Also the hand-set scenes of the aux tests, shared by the CPU and the GPU file.
"""
import numpy as np

import render_ref

NBODY = 9
BACKGROUND = 255
EMPTY = np.iinfo(np.uint64).max
# (camera, width, height, envs): drawn consecutively from one default_rng(0)
SCENE_SETS = (("top", 96, 72, 6), ("front_close", 64, 48, 3), ("angle", 37, 29, 2), ("top", 640, 480, 1))
# the bar of the GPU's depth against the float64 reference, relative: 4 x the largest of the per-set maxima of the
# float32 helper (on oracle32's frames) against the float64 helper (on oracle64's), measured on the CPU by
# test_render_aux_cpu.py: 1.4e-6 (top 96x72), 5.9e-5 (front_close, grazing faces), 2.5e-7 (angle), 2.1e-6 (640x480)
# (DESIGN.md 3.7 "Depth and labels")
DEPTH_REL_BAR = 2.36e-4


def scene_states():
    """[(camera, W, H, qpos float32 [n, 13])] of SCENE_SETS: per env arm uniform(-0.8, 0.8, 6), cube x
    uniform(-0.1, 0.3), y uniform(0.4, 0.8), z 0.01 + uniform(0, 0.05) and a normalised normal(size=4) quaternion."""
    rng = np.random.default_rng(0)
    out = []
    for cam, w, h, n in SCENE_SETS:
        q = np.zeros((n, 13))
        for i in range(n):
            q[i, :6] = rng.uniform(-0.8, 0.8, 6)
            q[i, 6] = rng.uniform(-0.1, 0.3)
            q[i, 7] = rng.uniform(0.4, 0.8)
            q[i, 8] = 0.01 + rng.uniform(0, 0.05)
            quat = rng.normal(size=4)
            q[i, 9:13] = quat / np.linalg.norm(quat)
        out.append((cam, w, h, q.astype(np.float32)))
    return out


def frames_of(o, m, qpos):
    """The oracle's body frames [(R, p)] and ee_site at qpos (forward kinematics only)."""
    d = o.new_data()
    o.reset(m, d, np.array(qpos[6:13], np.float64))
    for k in range(6):
        d.qpos[k] = float(qpos[k])
    o.call("so100o_fwd_position", m, d)
    fr = [(np.array(d.xmat[b][:], np.float64).reshape(3, 3), np.array(d.xpos[b][:], np.float64)) for b in range(NBODY)]
    return fr, np.array(d.site_ee[:], np.float64)


def _shade(cam, p, rgb8, dt):
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    n = np.where(ln > 0, n / np.where(ln > 0, ln, dt(1.0)), dt(0.0))
    v = cam["pos"][None, :] - p[:, 0]
    n = np.where((np.sum(n * v, axis=1) < 0)[:, None], -n, n)
    zc = cam["mat"][:, 2]
    lum = cam["head_ambient"] + cam["head_diffuse"] * np.maximum(dt(0.0), n @ zc)
    for d, c in zip(cam["light_dir"], cam["light_diffuse"]):
        lum = lum + c * np.maximum(dt(0.0), -(n @ d))
    base = np.stack([(rgb8 >> (8 * k)) & 0xFF for k in range(3)], axis=1).astype(dt) / dt(255.0)
    val = np.clip(base * lum[:, None], dt(0.0), dt(1.0))
    q = np.floor(val * dt(255.0) + dt(0.5)).astype(np.uint32)
    return q[:, 0] | (q[:, 1] << 8) | (q[:, 2] << 16)


def _tracking_frame(pos, target, dt):
    z = pos - target
    n = np.linalg.norm(z)
    z = z / n if n > 1e-15 else np.array([1.0, 0, 0], dt)
    x = np.cross(np.array([0.0, 0.0, 1.0], dt), z)
    n = np.linalg.norm(x)
    x = x / n if n > 1e-15 else np.array([1.0, 0, 0], dt)
    return np.stack([x, np.cross(z, x), z], axis=1).astype(dt)


def render(scene_tri, scene_body, scene_rgb, label, frames, cam, width, height, target=None, dtype=np.float64,
           winner=False):
    """frames: [NBODY] of (R [3,3], p [3]); label: uint8 [T]; cam: render_ref.camera_dict's dict; target: the tracked
    point of a tracking camera.  Returns (rgb uint8 [H,W,3], depth float32 [H,W], label uint8 [H,W]) and with
    winner=True a fourth, int32 [H,W]: the index of the triangle whose key the pixel holds (the first of equal keys),
    -1 on the background."""
    dt = np.dtype(dtype).type
    cam = dict(cam, pos=np.asarray(cam["pos"], dt), mat=np.asarray(cam["mat"], dt), fovy=dt(cam["fovy"]),
               znear=dt(cam["znear"]), head_ambient=dt(cam["head_ambient"]), head_diffuse=dt(cam["head_diffuse"]),
               light_dir=[np.asarray(d, dt) for d in cam["light_dir"]],
               light_diffuse=[dt(c) for c in cam["light_diffuse"]])
    if cam.get("track"):
        cam["mat"] = _tracking_frame(cam["pos"], np.asarray(target, dt), dt)
    R = np.stack([f[0] for f in frames]).astype(dt)[scene_body]
    P = np.stack([f[1] for f in frames]).astype(dt)[scene_body]
    w = np.einsum("tij,tvj->tvi", R, scene_tri.astype(dt)) + P[:, None, :]
    d = w - cam["pos"]
    c = d @ cam["mat"]
    depth = -c[..., 2]
    th = np.tan(dt(0.5) * np.radians(cam["fovy"]))
    aspect = dt(width) / dt(height)
    ok = np.all(depth > cam["znear"], axis=1)
    iz = dt(1.0) / np.where(depth > 0, depth, dt(1.0))
    sx = (c[..., 0] * iz / (th * aspect) * dt(0.5) + dt(0.5)) * dt(width)
    sy = (dt(0.5) - c[..., 1] * iz / th * dt(0.5)) * dt(height)
    col = _shade(cam, w, render_ref.pack_rgb(scene_rgb), dt)
    low = (col.astype(np.uint64) << np.uint64(8)) | np.asarray(label, np.uint64)
    key = np.full((height, width), EMPTY, np.uint64)
    win = np.full((height, width), -1, np.int32)
    half = dt(0.5)
    for t in np.nonzero(ok)[0]:
        x, y, z = sx[t], sy[t], iz[t]
        area = (x[1] - x[0]) * (y[2] - y[0]) - (x[2] - x[0]) * (y[1] - y[0])
        if not abs(area) > 1e-12:
            continue
        bx0, bx1 = max(0, int(np.floor(x.min() - half))), min(width - 1, int(np.ceil(x.max() - half)))
        by0, by1 = max(0, int(np.floor(y.min() - half))), min(height - 1, int(np.ceil(y.max() - half)))
        if bx0 > bx1 or by0 > by1:
            continue
        px, py = np.meshgrid(np.arange(bx0, bx1 + 1).astype(dt) + half, np.arange(by0, by1 + 1).astype(dt) + half)
        w0 = (x[2] - x[1]) * (py - y[1]) - (y[2] - y[1]) * (px - x[1])
        w1 = (x[0] - x[2]) * (py - y[2]) - (y[0] - y[2]) * (px - x[2])
        w2 = (x[1] - x[0]) * (py - y[0]) - (y[1] - y[0]) * (px - x[0])
        sg = dt(1.0) if area > 0 else dt(-1.0)
        inside = (w0 * sg >= 0) & (w1 * sg >= 0) & (w2 * sg >= 0)
        izp = (w0 * z[0] + w1 * z[1] + w2 * z[2]) / area
        inside &= izp > 0
        dep = (dt(1.0) / np.where(inside, izp, dt(1.0))).astype(np.float32)
        k = (dep.view(np.uint32).astype(np.uint64) << np.uint64(32)) | low[t]
        sub = key[by0:by1 + 1, bx0:bx1 + 1]
        np.copyto(win[by0:by1 + 1, bx0:bx1 + 1], np.int32(t), where=inside & (k < sub))
        np.copyto(sub, np.minimum(sub, k), where=inside)
    empty = key == EMPTY
    rgb = np.where(empty, np.uint64(0), (key >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.uint32)
    img = np.stack([(rgb >> (8 * k)) & 0xFF for k in range(3)], axis=-1).astype(np.uint8)
    dep = np.where(empty, np.uint64(0), key >> np.uint64(32)).astype(np.uint32).view(np.float32)
    lab = (key & np.uint64(0xFF)).astype(np.uint8)             # the empty key's low byte is 255
    return (img, dep, lab, win) if winner else (img, dep, lab)


_CACHE = {}


def reference(model, oracle, bits):
    """The helper's images of every scene of scene_states() in float`bits` arithmetic on `oracle`'s frames, computed
    once per session and shared (read only): [(camera, W, H, qpos, [(rgb, depth, label)] per env)]."""
    if bits in _CACHE:
        return _CACHE[bits]
    from gym_so100 import render as R
    scene = R.load_scene()
    lab, _ = R.segment_labels(scene)
    out = []
    for name, w, h, qpos in scene_states():
        cam = render_ref.camera_dict(R.make_camera(scene, name))
        imgs = []
        for q in qpos:
            fr, ee = frames_of(oracle, model, q.astype(np.float64))
            imgs.append(render(scene["tri"], scene["body"], scene["rgb"], lab, fr, cam, w, h, target=ee,
                               dtype=np.float64 if bits == 64 else np.float32))
        out.append((name, w, h, qpos, imgs))
    _CACHE[bits] = out
    return out
