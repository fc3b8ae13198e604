"""float64 numpy restatement of csrc/so100_views.hip's sampler (TEST INFRASTRUCTURE ONLY): the counter-based hash, the
ranges, the Rodrigues rotations and the colour quantisation of the per-env view records (include/so100.h so100_view,
so100_views_sample), plus the decoding of the [N, 40] dword records the device holds.

Every draw: U[0,1) = top 24 bits of splitmix64(splitmix64(seed ^ id * 0x100000001B3 ^ field * 0xD1B54A32D192ED03) +
episode) / 2^24, with the global env id, the env's episode number and the field numbers of include/so100.h."""
import numpy as np

NMAT, NLIGHT, WORDS = 5, 4, 40
M64 = 0xFFFFFFFFFFFFFFFF


def _splitmix64(x):
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def uniform(seed, ids, episode, field):
    """U[0,1) [N] for global env ids [N] (uint64) and episode numbers [N]."""
    ids = np.asarray(ids, dtype=np.uint64)
    ep = np.asarray(episode, dtype=np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    with np.errstate(over="ignore"):
        k = _splitmix64(np.uint64(seed & M64) ^ (ids * np.uint64(0x100000001B3)) ^
                        np.uint64(field * 0xD1B54A32D192ED03 & M64))
        k = _splitmix64(k + ep)
    return (k >> np.uint64(40)).astype(np.float64) / float(1 << 24)


def rodrigues(v):
    """[N,3] rotation vectors -> [N,3,3]: I + (sin t / t) K + (2 sin^2(t/2) / t^2) K^2."""
    v = np.asarray(v, np.float64)
    t2 = np.sum(v * v, axis=1)
    t = np.sqrt(t2)
    small = t <= 1e-12
    ts = np.where(small, 1.0, t)
    A = np.where(small, 1.0, np.sin(ts) / ts)
    B = np.where(small, 0.5, 2.0 * np.sin(0.5 * ts) ** 2 / np.where(small, 1.0, t2))
    K = np.zeros((len(v), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0] = -v[:, 2], v[:, 1], v[:, 2]
    K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -v[:, 0], -v[:, 1], v[:, 0]
    return np.eye(3)[None] + A[:, None, None] * K + B[:, None, None] * (K @ K)


def sample(dr, cam, base_rgb, ids, episode=None):
    """The records of global env ids `ids` in float64.  dr: _native.SO100ViewDR, cam: _native.SO100Camera (the base
    camera), base_rgb: [5] packed RGB8.  Returns a dict: pos [N,3], mat [N,3,3], fovy, head_ambient, head_diffuse [N],
    light_diffuse [N,4], light_dir [N,4,3], rgb [N,5] packed uint32, rgb_level [N,5,3] (val * 255 before the
    rounding: how near a half-integer a channel lies)."""
    ids = np.asarray(ids, dtype=np.uint64)
    n = len(ids)
    ep = np.zeros(n, np.int64) if episode is None else np.asarray(episode)
    seed = int(dr.seed)

    def u(field):
        return uniform(seed, ids, ep, field)

    def sym(field, hw):
        return (2.0 * u(field) - 1.0) * float(hw)

    def scale(pair, field):
        lo, hi = float(pair[0]), float(pair[1])
        return np.clip(lo + (hi - lo) * u(field), lo, hi)

    pos0 = np.array(cam.pos[:], np.float64)
    mat0 = np.array(cam.mat[:], np.float64).reshape(3, 3)
    out = {"pos": pos0[None] + np.stack([sym(16 + k, dr.cam_pos) for k in range(3)], axis=1)}
    R = rodrigues(np.stack([sym(19 + k, dr.cam_rot) for k in range(3)], axis=1))
    out["mat"] = mat0[None] @ R
    out["fovy"] = float(cam.fovy) * scale(dr.fovy, 22)
    out["head_ambient"] = float(cam.head_ambient) * scale(dr.ambient, 23)
    out["head_diffuse"] = float(cam.head_diffuse) * scale(dr.headlight, 24)
    L = rodrigues(np.stack([sym(29 + k, dr.light_rot) for k in range(3)], axis=1))
    d0 = np.array([cam.light_dir[l][:] for l in range(NLIGHT)], np.float64)             # [4,3]
    out["light_dir"] = np.einsum("nij,lj->nli", L, d0)
    out["light_diffuse"] = np.stack([float(cam.light_diffuse[l]) * scale(dr.light[l], 25 + l) for l in range(NLIGHT)],
                                    axis=1)
    level = np.zeros((n, NMAT, 3))
    for m in range(NMAT):
        for k in range(3):
            base = ((int(base_rgb[m]) >> (8 * k)) & 0xFF) / 255.0
            level[:, m, k] = np.clip(base * scale(dr.color[m], 32 + 3 * m + k), 0.0, 1.0) * 255.0
    q = np.floor(level + 0.5).astype(np.uint32)
    out["rgb_level"] = level
    out["rgb"] = q[..., 0] | (q[..., 1] << 8) | (q[..., 2] << 16)
    return out


def decode(words):
    """[N, 40] dwords (any 4-byte dtype) of so100_view records -> the dict of sample() (float32 values as float64)."""
    w = np.ascontiguousarray(words)
    assert w.ndim == 2 and w.shape[1] == WORDS and w.dtype.itemsize == 4
    f = w.view(np.float32).astype(np.float64)
    return {"pos": f[:, 0:3], "mat": f[:, 3:12].reshape(-1, 3, 3), "fovy": f[:, 12], "head_ambient": f[:, 13],
            "head_diffuse": f[:, 14], "light_diffuse": f[:, 15:19], "light_dir": f[:, 19:31].reshape(-1, 4, 3),
            "rgb": w.view(np.uint32)[:, 31:36].copy(), "reserved": w.view(np.uint32)[:, 36:40].copy()}


def camera_dict(rec, i, cam):
    """Env i's record as the camera dict tests/render_ref.py renders from (track, znear and nlight from cam)."""
    nl = int(cam.nlight)
    return {"pos": np.array(rec["pos"][i], np.float64), "mat": np.array(rec["mat"][i], np.float64),
            "track": int(cam.track), "fovy": float(rec["fovy"][i]), "znear": float(cam.znear),
            "head_ambient": float(rec["head_ambient"][i]), "head_diffuse": float(rec["head_diffuse"][i]),
            "light_dir": [np.array(rec["light_dir"][i][l], np.float64) for l in range(nl)],
            "light_diffuse": [float(rec["light_diffuse"][i][l]) for l in range(nl)]}


def triangle_rgb(rec, i, material):
    """Env i's per-triangle base colours [ntri, 3] in [0, 1] (what render_ref.render takes as scene_rgb): render_ref's
    pack_rgb maps byte / 255 back to the byte."""
    rgb = np.asarray(rec["rgb"][i], np.uint32)[np.asarray(material)]
    return np.stack([(rgb >> (8 * k)) & 0xFF for k in range(3)], axis=1).astype(np.float64) / 255.0


def faces_near_rounding(scene, material, rec, i, cam, frames, target, width, height, tol=1e-3):
    """(visible faces, how many of them have a channel whose shaded val * 255 lies within tol of a half-integer), for
    env i's record in the float64 reference alone: such a face may round to the other level in float32, a whole face
    off by one that a cap on the share of differing pixels would hide.  Visible = owns a pixel of the reference's
    image (tests/render_ref.py drawn with the triangle number as the unshaded colour)."""
    import render_ref
    cd = camera_dict(rec, i, cam)
    ids = np.arange(len(material), dtype=np.uint32) + 1
    id_rgb = np.stack([(ids >> (8 * k)) & 0xFF for k in range(3)], axis=1) / 255.0
    flat = dict(cd, head_ambient=1.0, head_diffuse=0.0, light_dir=[], light_diffuse=[])
    im = render_ref.render(scene["tri"], scene["body"], id_rgb, frames, flat, width, height, target=target)
    im = im.astype(np.uint32)
    vis = np.unique(im[..., 0] | (im[..., 1] << 8) | (im[..., 2] << 16))
    vis = vis[vis > 0] - 1
    if cd["track"]:
        cd = dict(cd, mat=render_ref.tracking_frame(cd["pos"], target))
    Rb = np.stack([f[0] for f in frames])[scene["body"]]
    Pb = np.stack([f[1] for f in frames])[scene["body"]]
    p = np.einsum("tij,tvj->tvi", Rb, scene["tri"].astype(np.float64)) + Pb[:, None, :]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    n = np.where(ln > 0, n / np.where(ln > 0, ln, 1.0), 0.0)
    n = np.where((np.sum(n * (cd["pos"][None] - p[:, 0]), axis=1) < 0)[:, None], -n, n)
    lum = cd["head_ambient"] + cd["head_diffuse"] * np.maximum(0.0, n @ cd["mat"][:, 2])
    for d, c in zip(cd["light_dir"], cd["light_diffuse"]):
        lum = lum + c * np.maximum(0.0, -(n @ d))
    level = np.clip(triangle_rgb(rec, i, material) * lum[:, None], 0.0, 1.0) * 255.0
    near = np.abs(level - np.floor(level) - 0.5) < tol
    return len(vis), int(near.any(axis=1)[vis].sum())
