"""ctypes binding of libso100_hip.so (include/so100.h).

The HIP library is the only compute path: if it cannot be loaded, every env constructor raises.
There is no CPU fallback in the product.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SO100_LIB") or os.path.join(HERE, "_lib", "libso100_hip.so")

SO100_FLAG_AUTORESET = 1
SO100_FLAG_DR = 2
SO100_DBG_OVF = 160                   # include/so100.h: the debug entries of contacts >= 16
SO100_DBG_STRIDE = 160 + 6 * (643 - 16)
TASKS = {"so100_cube_to_bin": 0, "so100_touch_cube": 1, "so100_touch_cube_sparse": 2, "so100_goal": 3}

_P = ctypes.c_void_p


class SO100Buffers(ctypes.Structure):
    """Mirror of ``so100_buffers`` (include/so100.h): device pointers, NULL = not requested."""
    _fields_ = [(n, _P) for n in (
        "qpos", "qvel", "qacc_warmstart", "elapsed", "episode", "action",
        "obs", "reward", "terminated", "truncated", "success", "final_obs", "diverged", "contact_bits",
        "achieved_goal", "desired_goal", "total_steps", "dr_params", "debug", "mocap", "reward64", "ncon_dropped",
        "ep_return", "ep_final", "ep_accum")]


SO100_MAX_LIGHTS = 4


class SO100Camera(ctypes.Structure):
    """Mirror of ``so100_camera`` (include/so100.h): pose, fovy, headlight and directional lights."""
    _fields_ = [("pos", ctypes.c_float * 3), ("mat", ctypes.c_float * 9), ("track", ctypes.c_int),
                ("fovy", ctypes.c_float),
                ("znear", ctypes.c_float), ("head_ambient", ctypes.c_float), ("head_diffuse", ctypes.c_float),
                ("nlight", ctypes.c_int), ("light_dir", (ctypes.c_float * 3) * SO100_MAX_LIGHTS),
                ("light_diffuse", ctypes.c_float * SO100_MAX_LIGHTS)]


class SO100ImageOut(ctypes.Structure):
    """Mirror of ``so100_image_out`` (include/so100.h): the sinks of one ``so100_render_to`` launch, NULL = not
    written.  ``size`` is set to the mirror's size, which the callee checks against its own."""
    _fields_ = [("size", ctypes.c_uint32), ("hwc", _P), ("chw", _P), ("flat", _P), ("flat_pitch", ctypes.c_int64)]

    def __init__(self, hwc=None, chw=None, flat=None, flat_pitch=0):
        super().__init__(ctypes.sizeof(SO100ImageOut), hwc, chw, flat, flat_pitch)


class SO100AuxOut(ctypes.Structure):
    """Mirror of ``so100_aux_out`` (include/so100.h): the depth and label sinks of one ``so100_render_aux`` launch,
    NULL = not written.  ``size`` is set to the mirror's size, which the callee checks against its own."""
    _fields_ = [("size", ctypes.c_uint32), ("depth", _P), ("label", _P)]

    def __init__(self, depth=None, label=None):
        super().__init__(ctypes.sizeof(SO100AuxOut), depth, label)


SO100_MAX_CAMS = 4


class SO100Cams(ctypes.Structure):
    """Mirror of ``so100_cams`` (include/so100.h): the cameras of one ``so100_render_cams`` launch and the body each
    rides on (0 = fixed in the world).  ``size`` is set to the mirror's size, which the callee checks against its own."""
    _fields_ = [("size", ctypes.c_uint32), ("ncam", ctypes.c_int32), ("cam", SO100Camera * SO100_MAX_CAMS),
                ("frame_body", ctypes.c_int32 * SO100_MAX_CAMS)]

    def __init__(self, cams=(), frame_body=()):
        super().__init__()
        self.size = ctypes.sizeof(SO100Cams)
        self.ncam = len(cams)
        for c, cam in enumerate(cams[:SO100_MAX_CAMS]):
            ctypes.memmove(ctypes.byref(self.cam[c]), ctypes.byref(cam), ctypes.sizeof(SO100Camera))
        for c, b in enumerate(frame_body[:SO100_MAX_CAMS]):
            self.frame_body[c] = int(b)


SO100_SHADOW_MAP_MAX = 64          # include/so100.h: the shadow map's largest side (it lives in LDS)


class SO100Shadow(ctypes.Structure):
    """Mirror of ``so100_shadow`` (include/so100.h): the casting light, the shadow map's size and placement, the depth
    bias and the optional mask sink of one ``so100_render_shadow`` launch.  ``size`` is set to the mirror's size, which
    the callee checks against its own."""
    _fields_ = [("size", ctypes.c_uint32), ("light", ctypes.c_int32), ("map_size", ctypes.c_int32),
                ("center", ctypes.c_float * 3), ("radius", ctypes.c_float), ("bias", ctypes.c_float),
                ("shadow_out", _P)]

    def __init__(self, light=-1, map_size=64, center=(0.0, 0.0, 0.0), radius=1.0, bias=0.0, shadow_out=None):
        super().__init__()
        self.size = ctypes.sizeof(SO100Shadow)
        self.light, self.map_size = int(light), int(map_size)
        self.center[:] = [float(x) for x in center]
        self.radius, self.bias = float(radius), float(bias)
        self.shadow_out = shadow_out


SO100_MSAA_MAX = 4                 # include/so100.h: the most samples per pixel of so100_render_msaa


class SO100Msaa(ctypes.Structure):
    """Mirror of ``so100_msaa`` (include/so100.h): the sample count and the samples' offsets from the pixel centre of one
    ``so100_render_msaa`` launch.  ``size`` is set to the mirror's size, which the callee checks against its own."""
    _fields_ = [("size", ctypes.c_uint32), ("samples", ctypes.c_int32),
                ("offset", (ctypes.c_float * 2) * SO100_MSAA_MAX)]

    def __init__(self, samples=1, offsets=((0.0, 0.0),)):
        super().__init__()
        self.size = ctypes.sizeof(SO100Msaa)
        self.samples = int(samples)
        for k, (x, y) in enumerate(list(offsets)[:SO100_MSAA_MAX]):
            self.offset[k][0], self.offset[k][1] = float(x), float(y)


class SO100EeCtrl(ctypes.Structure):
    """Mirror of ``so100_ee_ctrl`` (include/so100.h): the control record of one ``so100_ee_action`` launch.  ``size`` is
    set to the mirror's size, which the callee checks against its own."""
    _fields_ = [("size", ctypes.c_uint32), ("iters", ctypes.c_int32), ("pos_scale", ctypes.c_float),
                ("rot_scale", ctypes.c_float), ("damping", ctypes.c_float), ("dq_max", ctypes.c_float),
                ("lead_max", ctypes.c_float), ("ws_lo", ctypes.c_float * 3), ("ws_hi", ctypes.c_float * 3)]

    def __init__(self, iters=2, pos_scale=0.01, rot_scale=0.17453292, damping=0.02, dq_max=0.2, lead_max=0.5,
                 ws_lo=(0.0, 0.0, 0.0), ws_hi=(0.0, 0.0, 0.0)):
        super().__init__()
        self.size = ctypes.sizeof(SO100EeCtrl)
        self.iters = int(iters)
        self.pos_scale, self.rot_scale, self.damping = float(pos_scale), float(rot_scale), float(damping)
        self.dq_max, self.lead_max = float(dq_max), float(lead_max)
        self.ws_lo[:] = [float(x) for x in ws_lo]
        self.ws_hi[:] = [float(x) for x in ws_hi]


SO100_ACT_MAX_DELAY = 7            # include/so100.h: the longest actuation delay, control steps
SO100_ACT_HIST = 8                 # the command ring's slots


class SO100DrRanges(ctypes.Structure):
    """Mirror of ``so100_dr_ranges`` (include/so100.h): the ranges one ``so100_dr_sample`` launch draws the physical
    randomisation and the actuator records from.  The default is every range at zero width and off (scales 1, no delay,
    no smoothing, no slew limit); ``size`` is set to the mirror's size, which the callee checks against its own."""
    _fields_ = [("size", ctypes.c_uint32), ("reserved0", ctypes.c_uint32), ("seed", ctypes.c_uint64),
                ("mass", ctypes.c_float * 2), ("friction", ctypes.c_float * 2), ("delay", ctypes.c_int32 * 2),
                ("smoothing", ctypes.c_float * 2), ("rate", ctypes.c_float * 2)]

    def __init__(self, seed=0, mass=(1.0, 1.0), friction=(1.0, 1.0), delay=(0, 0), smoothing=(1.0, 1.0),
                 rate=(2.0, 2.0)):
        super().__init__()
        self.size = ctypes.sizeof(SO100DrRanges)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.mass[:] = [float(x) for x in mass]
        self.friction[:] = [float(x) for x in friction]
        self.delay[:] = [int(x) for x in delay]
        self.smoothing[:] = [float(x) for x in smoothing]
        self.rate[:] = [float(x) for x in rate]


SO100_NORM_MAX_DIM = 32            # include/so100.h: the columns one normaliser call carries
SO100_NORM_MAX_SRC = 3
SO100_NORM_INVERSE = 1
SO100_NORM_RET_UPDATE = 1
SO100_NORM_RET_NORMALIZE = 2


class SO100NormSrc(ctypes.Structure):
    """Mirror of ``so100_norm_src`` (include/so100.h): rows of float32 at (x, stride, offset, dim) and where
    ``so100_norm_apply`` writes them (y, y_stride)."""
    _fields_ = [("x", ctypes.c_void_p), ("y", ctypes.c_void_p), ("stride", ctypes.c_int32), ("offset", ctypes.c_int32),
                ("dim", ctypes.c_int32), ("y_stride", ctypes.c_int32)]


class SO100Norm(ctypes.Structure):
    """Mirror of ``so100_norm`` (include/so100.h): the sources and constants of one ``so100_norm_update`` /
    ``so100_norm_apply`` call.  ``sources``: up to three (x pointer, stride, offset, dim, y pointer, y_stride) tuples;
    ``size`` is set to the mirror's size, which the callee checks against its own."""
    _fields_ = [("size", ctypes.c_uint32), ("nsrc", ctypes.c_int32), ("epsilon", ctypes.c_double),
                ("clip", ctypes.c_double), ("flags", ctypes.c_uint32), ("reserved0", ctypes.c_uint32),
                ("src", SO100NormSrc * SO100_NORM_MAX_SRC)]

    def __init__(self, sources=(), epsilon=1e-8, clip=10.0, flags=0):
        super().__init__()
        self.size = ctypes.sizeof(SO100Norm)
        self.nsrc = len(sources)
        self.epsilon, self.clip, self.flags = float(epsilon), float(clip), int(flags)
        for k, (x, stride, offset, dim, y, y_stride) in enumerate(list(sources)[:SO100_NORM_MAX_SRC]):
            s = self.src[k]
            s.x, s.y = x, y
            s.stride, s.offset, s.dim, s.y_stride = int(stride), int(offset), int(dim), int(y_stride)


class SO100NormRet(ctypes.Structure):
    """Mirror of ``so100_norm_ret`` (include/so100.h): the constants of one ``so100_norm_return`` call."""
    _fields_ = [("size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("gamma", ctypes.c_double),
                ("epsilon", ctypes.c_double), ("clip", ctypes.c_double)]

    def __init__(self, flags=0, gamma=0.99, epsilon=1e-8, clip=10.0):
        super().__init__()
        self.size = ctypes.sizeof(SO100NormRet)
        self.flags = int(flags)
        self.gamma, self.epsilon, self.clip = float(gamma), float(epsilon), float(clip)


SO100_HER_FUTURE, SO100_HER_FINAL, SO100_HER_EPISODE = 0, 1, 2     # include/so100.h: so100_her.strategy
SO100_HER_MAX_ACTION = 16
HER_STRATEGIES = {"future": SO100_HER_FUTURE, "final": SO100_HER_FINAL, "episode": SO100_HER_EPISODE}
HER_ARRAYS = ("obs", "next_obs", "goal", "action", "reward", "terminated", "offset", "length", "meta", "stage_obs",
              "stage_goal", "prefix")
HER_STEP_INPUTS = ("prev_obs", "prev_goal", "obs", "final_obs", "goal", "action", "reward", "terminated", "truncated",
                   "diverged", "discard")
HER_OUTPUTS = ("observation", "achieved_goal", "desired_goal", "next_observation", "next_achieved_goal",
               "next_desired_goal", "actions", "rewards", "dones", "env", "slot", "goal_slot")


class SO100Her(ctypes.Structure):
    """Mirror of ``so100_her`` (include/so100.h): the shape, the sampling options and the device arrays of one hindsight
    replay buffer.  ``size`` is set to the mirror's size, which the callee checks against its own."""
    _fields_ = [("size", ctypes.c_uint32), ("n", ctypes.c_int32), ("T", ctypes.c_int32), ("action_dim", ctypes.c_int32),
                ("strategy", ctypes.c_int32), ("n_sampled_goal", ctypes.c_int32), ("seed", ctypes.c_uint64)] + \
               [(name, _P) for name in HER_ARRAYS]

    def __init__(self, n=0, T=1, action_dim=6, strategy=SO100_HER_FUTURE, n_sampled_goal=4, seed=0, **arrays):
        super().__init__()
        self.size = ctypes.sizeof(SO100Her)
        self.n, self.T, self.action_dim = int(n), int(T), int(action_dim)
        self.strategy, self.n_sampled_goal = int(strategy), int(n_sampled_goal)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        for name, p in arrays.items():
            if name not in HER_ARRAYS:
                raise TypeError(f"so100_her has no array {name!r}")
            setattr(self, name, p)


class SO100HerStep(ctypes.Structure):
    """Mirror of ``so100_her_step`` (include/so100.h): the device rows one ``so100_her_push`` reads."""
    _fields_ = [("size", ctypes.c_uint32), ("reserved0", ctypes.c_uint32)] + [(name, _P) for name in HER_STEP_INPUTS]

    def __init__(self, **inputs):
        super().__init__()
        self.size = ctypes.sizeof(SO100HerStep)
        for name, p in inputs.items():
            if name not in HER_STEP_INPUTS:
                raise TypeError(f"so100_her_step has no input {name!r}")
            setattr(self, name, p)


class SO100HerOut(ctypes.Structure):
    """Mirror of ``so100_her_out`` (include/so100.h): the device arrays one ``so100_her_sample`` fills."""
    _fields_ = [("size", ctypes.c_uint32), ("reserved0", ctypes.c_uint32)] + [(name, _P) for name in HER_OUTPUTS]

    def __init__(self, **outputs):
        super().__init__()
        self.size = ctypes.sizeof(SO100HerOut)
        for name, p in outputs.items():
            if name not in HER_OUTPUTS:
                raise TypeError(f"so100_her_out has no output {name!r}")
            setattr(self, name, p)


SO100_REPLAY_MAX_ACTION = 16      # include/so100.h
SO100_REPLAY_MAX_PAD = 64
REPLAY_ARRAYS = ("obs", "next_obs", "action", "reward", "terminated", "obs_img", "next_img", "meta", "prefix")
REPLAY_STEP_INPUTS = ("obs", "final_obs", "action", "reward", "terminated", "truncated", "diverged", "pixels",
                      "final_pixels")
REPLAY_OUTPUTS = ("obs", "next_obs", "actions", "rewards", "dones", "pixels", "next_pixels", "env", "slot", "shift")


class SO100Replay(ctypes.Structure):
    """Mirror of ``so100_replay`` (include/so100.h): the shape, the image layout, the sampling options and the device
    arrays of one uniform replay buffer.  ``size`` is set to the mirror's size, which the callee checks against its
    own."""
    _fields_ = [("size", ctypes.c_uint32), ("n", ctypes.c_int32), ("T", ctypes.c_int32), ("action_dim", ctypes.c_int32),
                ("planes", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("chan", ctypes.c_int32),
                ("P", ctypes.c_int32), ("pad", ctypes.c_int32), ("seed", ctypes.c_uint64)] + \
               [(name, _P) for name in REPLAY_ARRAYS]

    def __init__(self, n=0, T=2, action_dim=6, planes=0, H=0, W=0, chan=0, P=0, pad=0, seed=0, **arrays):
        super().__init__()
        self.size = ctypes.sizeof(SO100Replay)
        self.n, self.T, self.action_dim = int(n), int(T), int(action_dim)
        self.planes, self.H, self.W, self.chan, self.P = int(planes), int(H), int(W), int(chan), int(P)
        self.pad = int(pad)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        for name, p in arrays.items():
            if name not in REPLAY_ARRAYS:
                raise TypeError(f"so100_replay has no array {name!r}")
            setattr(self, name, p)


class SO100ReplayStep(ctypes.Structure):
    """Mirror of ``so100_replay_step`` (include/so100.h): the device rows one ``so100_replay_push`` reads."""
    _fields_ = [("size", ctypes.c_uint32), ("reserved0", ctypes.c_uint32)] + [(name, _P) for name in REPLAY_STEP_INPUTS]

    def __init__(self, **inputs):
        super().__init__()
        self.size = ctypes.sizeof(SO100ReplayStep)
        for name, p in inputs.items():
            if name not in REPLAY_STEP_INPUTS:
                raise TypeError(f"so100_replay_step has no input {name!r}")
            setattr(self, name, p)


class SO100ReplayOut(ctypes.Structure):
    """Mirror of ``so100_replay_out`` (include/so100.h): the device arrays one ``so100_replay_sample`` fills."""
    _fields_ = [("size", ctypes.c_uint32), ("reserved0", ctypes.c_uint32)] + [(name, _P) for name in REPLAY_OUTPUTS]

    def __init__(self, **outputs):
        super().__init__()
        self.size = ctypes.sizeof(SO100ReplayOut)
        for name, p in outputs.items():
            if name not in REPLAY_OUTPUTS:
                raise TypeError(f"so100_replay_out has no output {name!r}")
            setattr(self, name, p)


SO100_REPLAY_MAX_NSTEP = 16       # include/so100.h
REPLAY_NSTEP_OUTPUTS = ("discounts", "nsteps", "last_slot")


class SO100ReplayNstep(ctypes.Structure):
    """Mirror of ``so100_replay_nstep`` (include/so100.h): the window of an n-step sample and the ``ends`` array that the
    ``_nstep`` push and stage keep."""
    _fields_ = [("size", ctypes.c_uint32), ("n_step", ctypes.c_int32), ("gamma", ctypes.c_float),
                ("reserved0", ctypes.c_uint32), ("ends", _P)]

    def __init__(self, n_step=1, gamma=0.99, ends=None):
        super().__init__()
        self.size = ctypes.sizeof(SO100ReplayNstep)
        self.n_step, self.gamma, self.ends = int(n_step), float(gamma), ends


class SO100ReplayNstepOut(ctypes.Structure):
    """Mirror of ``so100_replay_nstep_out`` (include/so100.h): the device arrays one ``so100_replay_sample_nstep`` fills
    beside those of ``so100_replay_out``."""
    _fields_ = [("size", ctypes.c_uint32), ("reserved0", ctypes.c_uint32)] + [(name, _P) for name in REPLAY_NSTEP_OUTPUTS]

    def __init__(self, **outputs):
        super().__init__()
        self.size = ctypes.sizeof(SO100ReplayNstepOut)
        for name, p in outputs.items():
            if name not in REPLAY_NSTEP_OUTPUTS:
                raise TypeError(f"so100_replay_nstep_out has no output {name!r}")
            setattr(self, name, p)


SO100_REPLAY_PRIO_ONE = 65536    # include/so100.h: the fixed-point priority 1.0
REPLAY_PER_ARRAYS = ("prio", "sum", "max_prio")
REPLAY_PER_OUTPUTS = ("probs", "weights")


class SO100ReplayPer(ctypes.Structure):
    """Mirror of ``so100_replay_per`` (include/so100.h): the exponents of prioritised replay and its three arrays."""
    _fields_ = [("size", ctypes.c_uint32), ("alpha", ctypes.c_float), ("beta", ctypes.c_float), ("eps", ctypes.c_float),
                ("reserved", ctypes.c_uint32 * 2)] + [(name, _P) for name in REPLAY_PER_ARRAYS]

    def __init__(self, alpha=0.6, beta=0.4, eps=1e-6, **arrays):
        super().__init__()
        self.size = ctypes.sizeof(SO100ReplayPer)
        self.alpha, self.beta, self.eps = float(alpha), float(beta), float(eps)
        for name, p in arrays.items():
            if name not in REPLAY_PER_ARRAYS:
                raise TypeError(f"so100_replay_per has no array {name!r}")
            setattr(self, name, p)


class SO100ReplayPerOut(ctypes.Structure):
    """Mirror of ``so100_replay_per_out`` (include/so100.h): the device arrays one ``so100_replay_sample_per`` fills
    beside those of ``so100_replay_out`` (and ``so100_replay_nstep_out``)."""
    _fields_ = [("size", ctypes.c_uint32), ("reserved0", ctypes.c_uint32)] + [(name, _P) for name in REPLAY_PER_OUTPUTS]

    def __init__(self, **outputs):
        super().__init__()
        self.size = ctypes.sizeof(SO100ReplayPerOut)
        for name, p in outputs.items():
            if name not in REPLAY_PER_OUTPUTS:
                raise TypeError(f"so100_replay_per_out has no output {name!r}")
            setattr(self, name, p)


SO100_NMATERIAL = 5


class SO100View(ctypes.Structure):
    """Mirror of ``so100_view`` (include/so100.h): one env's camera pose, field of view, lights and the five materials'
    base colours for ``so100_render_views``; 40 dwords, device memory ([N, 40] int32 / float32 tensors)."""
    _fields_ = [("pos", ctypes.c_float * 3), ("mat", ctypes.c_float * 9), ("fovy", ctypes.c_float),
                ("head_ambient", ctypes.c_float), ("head_diffuse", ctypes.c_float),
                ("light_diffuse", ctypes.c_float * SO100_MAX_LIGHTS),
                ("light_dir", (ctypes.c_float * 3) * SO100_MAX_LIGHTS), ("rgb", ctypes.c_uint32 * SO100_NMATERIAL),
                ("reserved", ctypes.c_uint32 * 4)]


VIEW_WORDS = ctypes.sizeof(SO100View) // 4


class SO100ViewDR(ctypes.Structure):
    """Mirror of ``so100_view_dr`` (include/so100.h): the ranges ``so100_views_sample`` draws the records from.  The
    default is every range at zero width (the base view); ``size`` is set to the mirror's size, which the callee checks
    against its own."""
    _fields_ = [("size", ctypes.c_uint32), ("reserved0", ctypes.c_uint32), ("seed", ctypes.c_uint64),
                ("cam_pos", ctypes.c_float), ("cam_rot", ctypes.c_float), ("fovy", ctypes.c_float * 2),
                ("ambient", ctypes.c_float * 2), ("headlight", ctypes.c_float * 2),
                ("light", (ctypes.c_float * 2) * SO100_MAX_LIGHTS), ("light_rot", ctypes.c_float),
                ("color", (ctypes.c_float * 2) * SO100_NMATERIAL), ("reserved1", ctypes.c_float)]

    def __init__(self, seed=0):
        super().__init__()
        self.size = ctypes.sizeof(SO100ViewDR)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        for pair in (self.fovy, self.ambient, self.headlight, *self.light, *self.color):
            pair[0] = pair[1] = 1.0


class NativeLibraryError(RuntimeError):
    pass


_lib = None


ABI_VERSION = 25         # include/so100.h SO100_ABI_VERSION
HULL_CELLG = 8           # SO100_HULL_CELLG
HULL_NCELL = 6 * HULL_CELLG * HULL_CELLG
HULL_BLK = 16            # SO100_HULL_BLK
HULL_BLK_NONE = 0x7fffffff   # SO100_HULL_BLK_NONE


def load():
    """Load libso100_hip.so once; raise NativeLibraryError loudly if it is missing or broken."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryError(
            f"{LIB_PATH} not found: build it with `make -C gym-so100-c_amd/csrc` (or __graft_entry__.build()). "
            "The HIP kernels are the only compute path; there is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    lib.so100_abi_version.restype = ctypes.c_int
    lib.so100_last_error.restype = ctypes.c_char_p
    lib.so100_source_hash.restype = ctypes.c_char_p
    lib.so100_create.argtypes = [_P, ctypes.c_int, ctypes.c_int]
    lib.so100_create.restype = _P
    lib.so100_destroy.argtypes = [_P]
    lib.so100_num_envs.argtypes = [_P]
    lib.so100_configure.argtypes = [_P, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_int]
    lib.so100_reset.argtypes = [_P, ctypes.POINTER(SO100Buffers), _P, _P, _P]
    lib.so100_step.argtypes = [_P, ctypes.POINTER(SO100Buffers), ctypes.c_int, _P]
    lib.so100_goal_reward.argtypes = [_P, ctypes.c_int, _P, _P, _P, _P]
    lib.so100_eval_reward.argtypes = [_P, ctypes.c_int, ctypes.c_int, _P, _P, _P, _P, _P]
    lib.so100_spawn_pose.argtypes = [_P, ctypes.c_int, _P, _P, _P]
    lib.so100_unnormalize.argtypes = [_P, ctypes.c_int, _P, _P, _P]
    lib.so100_profile_enable.argtypes = [_P, ctypes.c_int]
    lib.so100_profile_read.argtypes = [_P, _P, _P, _P, _P]
    lib.so100_contact_count.argtypes = [_P, _P, _P]
    lib.so100_contact_counts.argtypes = [_P, _P, _P]
    lib.so100_pool_stats.argtypes = [_P, _P, ctypes.c_int]
    lib.so100_chunk_info.argtypes = [_P, _P, _P]
    lib.so100_set_step_mode.argtypes = [_P, ctypes.c_int]
    lib.so100_step_mode.argtypes = [_P]
    lib.so100_render_mesh.argtypes = [_P, _P, _P, _P, ctypes.c_int]
    lib.so100_render.argtypes = [_P, _P, _P, ctypes.POINTER(SO100Camera), ctypes.c_int, ctypes.c_int, _P, _P]
    lib.so100_render_to.argtypes = [_P, _P, _P, ctypes.POINTER(SO100Camera), ctypes.c_int, ctypes.c_int,
                                    ctypes.POINTER(SO100ImageOut), _P]
    lib.so100_view_bytes.argtypes = []
    lib.so100_render_materials.argtypes = [_P, _P, ctypes.c_int]
    lib.so100_render_views.argtypes = [_P, _P, _P, ctypes.POINTER(SO100Camera), _P, ctypes.c_int, ctypes.c_int,
                                       ctypes.POINTER(SO100ImageOut), _P]
    lib.so100_views_sample.argtypes = [_P, ctypes.POINTER(SO100ViewDR), ctypes.POINTER(SO100Camera), _P, _P, _P, _P, _P]
    lib.so100_aux_out_bytes.argtypes = []
    lib.so100_render_labels.argtypes = [_P, _P, ctypes.c_int]
    lib.so100_render_aux.argtypes = [_P, _P, _P, ctypes.POINTER(SO100Camera), _P, ctypes.c_int, ctypes.c_int,
                                     ctypes.POINTER(SO100ImageOut), ctypes.POINTER(SO100AuxOut), _P]
    lib.so100_cams_bytes.argtypes = []
    lib.so100_render_cams.argtypes = [_P, _P, _P, ctypes.POINTER(SO100Cams), _P, ctypes.c_int, ctypes.c_int,
                                      ctypes.POINTER(SO100ImageOut), ctypes.POINTER(SO100AuxOut), _P]
    lib.so100_shadow_bytes.argtypes = []
    lib.so100_render_casters.argtypes = [_P, _P, ctypes.c_int]
    lib.so100_render_shadow.argtypes = [_P, _P, _P, ctypes.POINTER(SO100Cams), _P, ctypes.c_int, ctypes.c_int,
                                        ctypes.POINTER(SO100ImageOut), ctypes.POINTER(SO100AuxOut),
                                        ctypes.POINTER(SO100Shadow), _P]
    lib.so100_msaa_bytes.argtypes = []
    lib.so100_render_msaa.argtypes = [_P, _P, _P, ctypes.POINTER(SO100Cams), _P, ctypes.c_int, ctypes.c_int,
                                      ctypes.POINTER(SO100ImageOut), ctypes.POINTER(SO100Msaa), _P]
    lib.so100_ee_ctrl_bytes.argtypes = []
    lib.so100_ee_action.argtypes = [_P, ctypes.POINTER(SO100EeCtrl), _P, _P, _P, _P, _P, _P, _P]
    lib.so100_ee_jacobian.argtypes = [_P, ctypes.c_int, _P, _P, _P, _P]
    lib.so100_dr_ranges_bytes.argtypes = []
    lib.so100_dr_sample.argtypes = [_P, ctypes.POINTER(SO100DrRanges), _P, _P, _P, _P, _P, _P]
    lib.so100_actuate.argtypes = [_P, _P, _P, _P, _P, _P, _P, _P, _P]
    lib.so100_norm_bytes.argtypes = []
    lib.so100_norm_ret_bytes.argtypes = []
    lib.so100_norm_limits.argtypes = [_P, _P]
    lib.so100_norm_work_bytes.argtypes = [ctypes.c_int]
    lib.so100_norm_update.argtypes = [_P, ctypes.POINTER(SO100Norm), ctypes.c_int, _P, _P, _P, _P]
    lib.so100_norm_apply.argtypes = [_P, ctypes.POINTER(SO100Norm), ctypes.c_int, _P, _P, _P]
    lib.so100_norm_return.argtypes = [_P, ctypes.POINTER(SO100NormRet), ctypes.c_int, _P, _P, _P, _P, _P, _P, _P, _P]
    lib.so100_her_bytes.argtypes = []
    lib.so100_her_step_bytes.argtypes = []
    lib.so100_her_out_bytes.argtypes = []
    lib.so100_her_limits.argtypes = [_P, _P]
    lib.so100_her_storage_bytes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.so100_her_storage_bytes.restype = ctypes.c_int64
    lib.so100_her_push.argtypes = [_P, ctypes.POINTER(SO100Her), ctypes.POINTER(SO100HerStep), _P]
    lib.so100_her_discard.argtypes = [_P, ctypes.POINTER(SO100Her), _P, _P, _P, _P]
    lib.so100_her_scan.argtypes = [_P, ctypes.POINTER(SO100Her), _P]
    lib.so100_her_sample.argtypes = [_P, ctypes.POINTER(SO100Her), ctypes.c_int, ctypes.c_uint64,
                                     ctypes.POINTER(SO100HerOut), _P]
    lib.so100_replay_bytes.argtypes = []
    lib.so100_replay_step_bytes.argtypes = []
    lib.so100_replay_out_bytes.argtypes = []
    lib.so100_replay_storage_bytes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.so100_replay_storage_bytes.restype = ctypes.c_int64
    lib.so100_replay_push.argtypes = [_P, ctypes.POINTER(SO100Replay), ctypes.POINTER(SO100ReplayStep), _P]
    lib.so100_replay_stage.argtypes = [_P, ctypes.POINTER(SO100Replay), _P, _P, _P, _P]
    lib.so100_replay_scan.argtypes = [_P, ctypes.POINTER(SO100Replay), _P]
    lib.so100_replay_sample.argtypes = [_P, ctypes.POINTER(SO100Replay), ctypes.c_int, ctypes.c_uint64,
                                        ctypes.POINTER(SO100ReplayOut), _P]
    lib.so100_replay_nstep_bytes.argtypes = []
    lib.so100_replay_nstep_out_bytes.argtypes = []
    lib.so100_replay_nstep_storage_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.so100_replay_nstep_storage_bytes.restype = ctypes.c_int64
    lib.so100_replay_push_nstep.argtypes = [_P, ctypes.POINTER(SO100Replay), ctypes.POINTER(SO100ReplayNstep),
                                            ctypes.POINTER(SO100ReplayStep), _P]
    lib.so100_replay_stage_nstep.argtypes = [_P, ctypes.POINTER(SO100Replay), ctypes.POINTER(SO100ReplayNstep), _P, _P,
                                             _P, _P]
    lib.so100_replay_sample_nstep.argtypes = [_P, ctypes.POINTER(SO100Replay), ctypes.POINTER(SO100ReplayNstep),
                                              ctypes.c_int, ctypes.c_uint64, ctypes.POINTER(SO100ReplayOut),
                                              ctypes.POINTER(SO100ReplayNstepOut), _P]
    lib.so100_replay_per_bytes.argtypes = []
    lib.so100_replay_per_out_bytes.argtypes = []
    lib.so100_replay_per_storage_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.so100_replay_per_storage_bytes.restype = ctypes.c_int64
    lib.so100_replay_push_per.argtypes = [_P, ctypes.POINTER(SO100Replay), ctypes.POINTER(SO100ReplayPer),
                                          ctypes.POINTER(SO100ReplayNstep), ctypes.POINTER(SO100ReplayStep), _P]
    lib.so100_replay_per_scan.argtypes = [_P, ctypes.POINTER(SO100Replay), ctypes.POINTER(SO100ReplayPer), _P]
    lib.so100_replay_sample_per.argtypes = [_P, ctypes.POINTER(SO100Replay), ctypes.POINTER(SO100ReplayPer),
                                            ctypes.POINTER(SO100ReplayNstep), ctypes.c_int, ctypes.c_uint64,
                                            ctypes.POINTER(SO100ReplayOut), ctypes.POINTER(SO100ReplayNstepOut),
                                            ctypes.POINTER(SO100ReplayPerOut), _P]
    lib.so100_replay_per_update.argtypes = [_P, ctypes.POINTER(SO100Replay), ctypes.POINTER(SO100ReplayPer),
                                            ctypes.c_int, _P, _P, _P, _P]
    lib.so100_hull_cells.argtypes = [_P, _P, _P, ctypes.c_int]
    lib.so100_hull_blocks.argtypes = [_P, _P, ctypes.c_int]
    lib.so100_hull_support_probe.argtypes = [_P, ctypes.c_int, _P, ctypes.c_int, ctypes.c_int, _P]
    lib.so100_set_fused_build.argtypes = [_P, ctypes.c_int]
    lib.so100_fused_build.argtypes = [_P, ctypes.c_int]
    lib.so100_set_env_packing.argtypes = [_P, ctypes.c_int]
    lib.so100_env_packing.argtypes = [_P]
    lib.so100_env_order.argtypes = [_P, _P, ctypes.c_int]
    lib.so100_env_cost.argtypes = [_P, _P, ctypes.c_int]
    lib.so100_wave_cost.argtypes = [_P, _P, ctypes.c_int]
    for fn in ("so100_destroy", "so100_num_envs", "so100_configure", "so100_reset", "so100_step",
               "so100_goal_reward", "so100_eval_reward", "so100_spawn_pose", "so100_unnormalize",
               "so100_profile_enable", "so100_profile_read", "so100_contact_count", "so100_contact_counts",
               "so100_pool_stats", "so100_chunk_info", "so100_render_mesh", "so100_render", "so100_render_to", "so100_set_step_mode", "so100_step_mode", "so100_hull_cells",
               "so100_set_fused_build", "so100_fused_build", "so100_set_env_packing", "so100_env_packing",
               "so100_env_order", "so100_env_cost", "so100_wave_cost", "so100_view_bytes", "so100_render_materials",
               "so100_render_views", "so100_views_sample", "so100_aux_out_bytes", "so100_render_labels",
               "so100_render_aux", "so100_cams_bytes", "so100_render_cams", "so100_shadow_bytes",
               "so100_render_casters", "so100_render_shadow", "so100_msaa_bytes", "so100_render_msaa",
               "so100_ee_ctrl_bytes", "so100_ee_action", "so100_ee_jacobian", "so100_hull_blocks",
               "so100_hull_support_probe", "so100_dr_ranges_bytes", "so100_dr_sample", "so100_actuate",
               "so100_norm_bytes", "so100_norm_ret_bytes", "so100_norm_limits", "so100_norm_work_bytes",
               "so100_norm_update", "so100_norm_apply", "so100_norm_return", "so100_her_bytes",
               "so100_her_step_bytes", "so100_her_out_bytes", "so100_her_limits", "so100_her_push",
               "so100_her_discard", "so100_her_scan", "so100_her_sample", "so100_replay_bytes",
               "so100_replay_step_bytes", "so100_replay_out_bytes", "so100_replay_push", "so100_replay_stage",
               "so100_replay_scan", "so100_replay_sample", "so100_replay_nstep_bytes", "so100_replay_nstep_out_bytes",
               "so100_replay_push_nstep", "so100_replay_stage_nstep", "so100_replay_sample_nstep",
               "so100_replay_per_bytes", "so100_replay_per_out_bytes", "so100_replay_push_per", "so100_replay_per_scan",
               "so100_replay_sample_per", "so100_replay_per_update"):
        getattr(lib, fn).restype = ctypes.c_int
    lib.so100_struct_sizes.argtypes = [_P, _P]
    lib.so100_struct_sizes.restype = ctypes.c_int
    if lib.so100_abi_version() != ABI_VERSION:
        raise NativeLibraryError("libso100_hip.so ABI mismatch")
    mb, bb = ctypes.c_int(0), ctypes.c_int(0)
    lib.so100_struct_sizes(ctypes.byref(mb), ctypes.byref(bb))
    from .model import SO100Model
    if mb.value != ctypes.sizeof(SO100Model) or bb.value != ctypes.sizeof(SO100Buffers):
        raise NativeLibraryError(f"struct layout mismatch: so100_model {mb.value} vs {ctypes.sizeof(SO100Model)}, "
                                 f"so100_buffers {bb.value} vs {ctypes.sizeof(SO100Buffers)}")
    if lib.so100_view_bytes() != ctypes.sizeof(SO100View):
        raise NativeLibraryError(f"struct layout mismatch: so100_view {lib.so100_view_bytes()} vs "
                                 f"{ctypes.sizeof(SO100View)}")
    if lib.so100_aux_out_bytes() != ctypes.sizeof(SO100AuxOut):
        raise NativeLibraryError(f"struct layout mismatch: so100_aux_out {lib.so100_aux_out_bytes()} vs "
                                 f"{ctypes.sizeof(SO100AuxOut)}")
    if lib.so100_cams_bytes() != ctypes.sizeof(SO100Cams):
        raise NativeLibraryError(f"struct layout mismatch: so100_cams {lib.so100_cams_bytes()} vs "
                                 f"{ctypes.sizeof(SO100Cams)}")
    if lib.so100_shadow_bytes() != ctypes.sizeof(SO100Shadow):
        raise NativeLibraryError(f"struct layout mismatch: so100_shadow {lib.so100_shadow_bytes()} vs "
                                 f"{ctypes.sizeof(SO100Shadow)}")
    if lib.so100_msaa_bytes() != ctypes.sizeof(SO100Msaa):
        raise NativeLibraryError(f"struct layout mismatch: so100_msaa {lib.so100_msaa_bytes()} vs "
                                 f"{ctypes.sizeof(SO100Msaa)}")
    if lib.so100_ee_ctrl_bytes() != ctypes.sizeof(SO100EeCtrl):
        raise NativeLibraryError(f"struct layout mismatch: so100_ee_ctrl {lib.so100_ee_ctrl_bytes()} vs "
                                 f"{ctypes.sizeof(SO100EeCtrl)}")
    if lib.so100_dr_ranges_bytes() != ctypes.sizeof(SO100DrRanges):
        raise NativeLibraryError(f"struct layout mismatch: so100_dr_ranges {lib.so100_dr_ranges_bytes()} vs "
                                 f"{ctypes.sizeof(SO100DrRanges)}")
    if lib.so100_norm_bytes() != ctypes.sizeof(SO100Norm) or lib.so100_norm_ret_bytes() != ctypes.sizeof(SO100NormRet):
        raise NativeLibraryError(f"struct layout mismatch: so100_norm {lib.so100_norm_bytes()} vs "
                                 f"{ctypes.sizeof(SO100Norm)}, so100_norm_ret {lib.so100_norm_ret_bytes()} vs "
                                 f"{ctypes.sizeof(SO100NormRet)}")
    for fn, mirror in (("so100_her_bytes", SO100Her), ("so100_her_step_bytes", SO100HerStep),
                       ("so100_her_out_bytes", SO100HerOut), ("so100_replay_bytes", SO100Replay),
                       ("so100_replay_step_bytes", SO100ReplayStep), ("so100_replay_out_bytes", SO100ReplayOut),
                       ("so100_replay_nstep_bytes", SO100ReplayNstep),
                       ("so100_replay_nstep_out_bytes", SO100ReplayNstepOut),
                       ("so100_replay_per_bytes", SO100ReplayPer), ("so100_replay_per_out_bytes", SO100ReplayPerOut)):
        if getattr(lib, fn)() != ctypes.sizeof(mirror):
            raise NativeLibraryError(f"struct layout mismatch: {fn} {getattr(lib, fn)()} vs {ctypes.sizeof(mirror)}")
    _lib = lib
    return lib


def norm_limits():
    """(rows a workgroup of the moments kernel takes below the grid cap, the grid cap) (so100_norm_limits)."""
    r, g = ctypes.c_int(0), ctypes.c_int(0)
    check(load().so100_norm_limits(ctypes.byref(r), ctypes.byref(g)), "so100_norm_limits")
    return r.value, g.value


def her_limits():
    """(the scan's workgroup size, the elements one pass of it takes) (so100_her_limits)."""
    w, t = ctypes.c_int(0), ctypes.c_int(0)
    check(load().so100_her_limits(ctypes.byref(w), ctypes.byref(t)), "so100_her_limits")
    return w.value, t.value


EXPORTED_SYMBOLS = ("so100_abi_version", "so100_last_error", "so100_source_hash", "so100_struct_sizes", "so100_create", "so100_destroy", "so100_num_envs",
                    "so100_configure", "so100_reset", "so100_step", "so100_goal_reward", "so100_eval_reward",
                    "so100_spawn_pose", "so100_unnormalize", "so100_profile_enable", "so100_profile_read",
                    "so100_contact_count", "so100_contact_counts", "so100_pool_stats", "so100_chunk_info", "so100_render_mesh",
                    "so100_render", "so100_render_to",
                    "so100_set_step_mode", "so100_step_mode", "so100_hull_cells", "so100_set_fused_build",
                    "so100_fused_build", "so100_set_env_packing", "so100_env_packing", "so100_env_order",
                    "so100_env_cost", "so100_wave_cost", "so100_view_bytes", "so100_render_materials",
                    "so100_render_views", "so100_views_sample", "so100_aux_out_bytes", "so100_render_labels",
                    "so100_render_aux", "so100_cams_bytes", "so100_render_cams", "so100_shadow_bytes",
                    "so100_render_casters", "so100_render_shadow", "so100_msaa_bytes", "so100_render_msaa",
                    "so100_ee_ctrl_bytes", "so100_ee_action", "so100_ee_jacobian", "so100_hull_blocks",
                    "so100_hull_support_probe", "so100_dr_ranges_bytes", "so100_dr_sample", "so100_actuate",
                    "so100_norm_bytes", "so100_norm_ret_bytes", "so100_norm_limits", "so100_norm_work_bytes",
                    "so100_norm_update", "so100_norm_apply", "so100_norm_return", "so100_her_bytes",
                    "so100_her_step_bytes", "so100_her_out_bytes", "so100_her_limits", "so100_her_storage_bytes",
                    "so100_her_push", "so100_her_discard", "so100_her_scan", "so100_her_sample", "so100_replay_bytes",
                    "so100_replay_step_bytes", "so100_replay_out_bytes", "so100_replay_storage_bytes",
                    "so100_replay_push", "so100_replay_stage", "so100_replay_scan", "so100_replay_sample",
                    "so100_replay_nstep_bytes", "so100_replay_nstep_out_bytes", "so100_replay_nstep_storage_bytes",
                    "so100_replay_push_nstep", "so100_replay_stage_nstep", "so100_replay_sample_nstep",
                    "so100_replay_per_bytes", "so100_replay_per_out_bytes", "so100_replay_per_storage_bytes",
                    "so100_replay_push_per", "so100_replay_per_scan", "so100_replay_sample_per",
                    "so100_replay_per_update")


def source_hash():
    """The content hash of the sources the loaded library was built from (so100_source_hash)."""
    return load().so100_source_hash().decode()


def check(rc, what):
    if rc != 0:
        msg = load().so100_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed ({rc}): {msg}")


def ptr(t):
    """Device pointer of a torch tensor (or None -> NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream_ptr(torch_mod, device):
    s = torch_mod.cuda.current_stream(device)
    return ctypes.c_void_p(s.cuda_stream)
