"""numpy restatement of the mounted-camera frame of csrc/so100_render_cams.hip (TEST INFRASTRUCTURE ONLY).

A camera of so100_cams with frame_body = b > 0 holds pos (and, without tracking, mat) in body b's frame.  Per env:
pos_w = R_b pos + p_b; with track = 1 the frame is the targetbody rule from pos_w to ee_site, with track = 0 it is
R_b mat, a rigid mount.  ``world_camera`` does that and nothing else; the image is then render_aux_ref.render's of the
resulting world camera.  The states are render_aux_ref.scene_states()'s 12, all drawn at 64x48 here.

The two mounted cameras of the tests: ``left_wrist`` (render.MOUNTED_CAMERAS: Fixed_Jaw, pos (0, 0, 0.55), fovy 20,
tracking) and RIGID, a fixed mount on the same link.  RIGID's mat is the targetbody frame of its position towards the
arm's ee_site at the zero arm pose, expressed in Fixed_Jaw's frame and rounded to 4 decimals (the kernel and this file
use the same nine numbers), so it looks along the gripper as left_wrist does at that pose and swings with the link
elsewhere.  On the 12 states its float32-against-float64 images differ in no label and no colour, the foreground covers
5-40 % of every image and the largest relative depth error is 7.7e-6 (test_render_cams_cpu.py asserts the acceptance).
"""
import numpy as np

import render_aux_ref as A
import render_ref

W, H = 64, 48
DEPTH_REL_BAR = A.DEPTH_REL_BAR          # the wrist sets' float32 maximum is inside 5.9e-5 (test_render_cams_cpu.py)
RIGID = dict(body=6, pos=(0.0, 0.0, 0.3), fovy=70.0,
             mat=((0.0, -1.0, 0.0), (0.9806, 0.0, 0.1961), (-0.1961, 0.0, 0.9806)))


def states():
    """float32 [12, 13]: the states of every set of render_aux_ref.scene_states(), in order."""
    return np.concatenate([s[3] for s in A.scene_states()]).astype(np.float32)


def world_camera(cam, frame_body, frames, dtype=np.float64):
    """cam: render_ref.camera_dict's dict with pos / mat in body `frame_body`'s frame (0: the world, returned as it is);
    frames: [NBODY] of (R, p).  Returns the dict of the camera in the world, in `dtype` arithmetic."""
    if frame_body == 0:
        return cam
    dt = np.dtype(dtype).type
    R, p = (np.asarray(x).astype(dt) for x in frames[frame_body])
    out = dict(cam, pos=R @ np.asarray(cam["pos"]).astype(dt) + p)
    if not cam.get("track"):
        out["mat"] = R @ np.asarray(cam["mat"]).astype(dt)
    return out


def mounted_cameras(R_mod, scene):
    """{name: (so100_camera, frame_body)} of the two mounted cameras under test."""
    wrist = R_mod.camera_by_name(scene, "left_wrist")
    rigid = R_mod.make_mounted_camera(scene, RIGID["body"], RIGID["pos"], mat=np.array(RIGID["mat"]),
                                      fovy=RIGID["fovy"])
    return {"left_wrist": (wrist, wrist.frame_body), "rigid": (rigid, rigid.frame_body)}


_CACHE = {}


def reference(model, oracle, bits, name):
    """[(rgb, depth, label)] per state: camera `name` ("left_wrist" / "rigid") at 64x48 in float`bits` arithmetic on
    `oracle`'s frames; computed once per session and shared (read only)."""
    if (bits, name) in _CACHE:
        return _CACHE[(bits, name)]
    from gym_so100 import render as R
    scene = R.load_scene()
    lab, _ = R.segment_labels(scene)
    cam, fb = mounted_cameras(R, scene)[name]
    dtype = np.float64 if bits == 64 else np.float32
    out = []
    for q in states():
        fr, ee = A.frames_of(oracle, model, q.astype(np.float64))
        wc = world_camera(render_ref.camera_dict(cam), fb, fr, dtype)
        out.append(A.render(scene["tri"], scene["body"], scene["rgb"], lab, fr, wc, W, H, target=ee, dtype=dtype))
    _CACHE[(bits, name)] = out
    return out
