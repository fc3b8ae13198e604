"""so100_render_to (ABI 19: one render launch, several sinks) without a device: the argument checks that come before
any device call, and the ctypes mirror of so100_image_out against the callee's own sizeof."""
import ctypes
import os
import re

from gym_so100 import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def call(lib, sinks):
    cam = _native.SO100Camera()
    rc = lib.so100_render_to(None, None, None, ctypes.byref(cam), 8, 8, ctypes.byref(sinks), None)
    return rc, lib.so100_last_error()


def test_render_to_rejects_a_null_env_with_its_text():
    lib = _native.load()
    assert "so100_render_to" in _native.EXPORTED_SYMBOLS and _native.ABI_VERSION >= 19
    rc, err = call(lib, _native.SO100ImageOut(hwc=1 << 20))     # never dereferenced: the env check comes first
    assert rc != 0 and b"so100_render_to: NULL env" in err


def test_image_out_mirror_has_the_size_the_callee_accepts():
    """The callee compares so100_image_out.size with its own sizeof before anything else: the mirror's size passes
    that check (the call goes on to refuse the NULL env), any other size is refused by it."""
    lib = _native.load()
    s = _native.SO100ImageOut(hwc=1 << 20)
    assert s.size == ctypes.sizeof(_native.SO100ImageOut)
    rc, err = call(lib, s)
    assert rc != 0 and b"NULL env" in err and b"size" not in err
    for wrong in (0, s.size - 8, s.size + 8):
        s.size = wrong
        rc, err = call(lib, s)
        assert rc != 0 and b"so100_image_out.size %d, expected %d" % (wrong, ctypes.sizeof(s)) in err, err


def test_image_out_mirror_follows_the_header():
    src = open(os.path.join(ROOT, "include", "so100.h")).read()
    body = re.search(r"typedef struct so100_image_out \{(.*?)\} so100_image_out;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = [re.sub(r"\s+", " ", d.strip()) for d in body.split(";") if d.strip()]
    assert decl == ["uint32_t size", "uint8_t* hwc", "uint8_t* chw", "float* flat", "int64_t flat_pitch"]
    assert [f[0] for f in _native.SO100ImageOut._fields_] == [d.split()[-1] for d in decl]
