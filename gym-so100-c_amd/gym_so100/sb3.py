"""stable-baselines3 VecEnv adapter over SO100VecEnv.

The reference's training scripts drive gym_so100 through SB3: ``make_vec_env(..., SubprocVecEnv)`` +
``VecNormalize`` (reference scripts/train_sac.py:294-310) and ``DummyVecEnv`` + ``HerReplayBuffer``
for the GoalEnv (scripts/train_sac_her.py:231-251).  ``SO100SB3VecEnv`` is a drop-in for those
vectorised envs: one object stepping N envs on the GPU with SB3's VecEnv contract:

* ``reset() -> obs`` (numpy, or a dict of numpy arrays for the GoalEnv), seeded by ``seed(s)`` as
  SB3 does (env i <- s + i, one-shot);
* ``step_async(actions)`` / ``step_wait() -> (obs, rewards, dones, infos)`` with ``dones = terminated
  | truncated`` and SB3's auto-reset conventions per done env: ``infos[i]["terminal_observation"]``
  (the finished episode's last observation) and ``infos[i]["TimeLimit.truncated"]`` (truncated and not
  terminated); every info carries ``is_success``;
* ``env_method("compute_reward", achieved, desired, infos)`` for HER (batched, on the device);
* ``get_attr`` / ``set_attr`` / ``env_is_wrapped`` / ``seed`` / ``close`` / ``get_images``.

When stable-baselines3 is importable the class derives from its ``VecEnv`` (so ``VecNormalize`` and
``isinstance`` checks accept it); otherwise it is a duck-typed equivalent.  The physics stays on the
GPU; this layer only moves the observation and the per-env scalars to host numpy, which SB3's
numpy interface requires.

``obs_type="so100_pixels_agent_pos"`` is the observation the reference's scripts train on (train_sac.py:294-310):

* the three arm tasks observe ``{"pixels": uint8 [H,W,3], "agent_pos": float32 [6]}`` (reference env.py:50-66).
  With ``channels_first=True`` the image is [3,H,W], drawn in that layout by the render kernel, so the script's
  ``VecTransposeImage`` line is dropped; with the default the reference's wrapper stack applies as written;
* the GoalEnv observes ``"observation"`` = the flattened image / 255 followed by agent_pos, float32 [3HW+6]
  (env.py:219-238, 267-270), filled on the device by the render launch (``SO100VecEnv(flat_pixels=True)``).

``cameras=("top", "left_wrist")`` (K names of render.CAMERAS / render.MOUNTED_CAMERAS) observes K cameras drawn by one
launch: the arm tasks, which then need ``channels_first=True``, emit ``pixels`` as uint8 [3K,H,W], the channel-stacked
image SB3's CNN takes (a free reshape of the env's [N,K,3,H,W]); the GoalEnv emits float32 [K*3HW+6].

``shadows=True`` (or a dict, render.SHADOW_KEYS) is forwarded to the env: the images then carry the cast shadows of the
scene's shadow-casting light, drawn in the same launch, with no further host copy.  The shadow mask is not forwarded.

``antialias=True`` (or 2 / 4, or a dict, render.AA_KEYS) is forwarded to the env: the images are then multisampled and
resolved inside the render launch, with no further host copy.

``action_mode="ee_delta"`` (and ``ee_control``) is forwarded to the env: the action space is then ``Box(-1, 1, (5,))``,
the Cartesian delta (dx, dy, dz, droll, grip) a device prologue turns into the joint actions of the unchanged step.

``domain_randomization`` is handed to the env as it is, its ``per_episode`` and ``actuation`` keys included (physical
parameters drawn again for every new episode; a per-env actuation delay, smoothing and slew limit between the action and
the step): both run on the device, and the adapter's contract does not change.

``normalize=True`` (or a dict, normalize.NORMALIZE_DEFAULTS) is forwarded to the env and replaces the scripts'
``VecNormalize(env, norm_obs=True, norm_reward=False, clip_obs=10.0)`` line: the running statistics live and are applied
on the device, and the adapter hands out the normalised observations, rewards and
``terminal_observation``.  It carries VecNormalize's surface: ``obs_rms`` / ``ret_rms`` (assignable:
``eval_env.obs_rms = train_env.obs_rms``), ``training``, ``norm_reward``, ``get_original_obs()``,
``get_original_reward()``, ``normalize_obs`` / ``unnormalize_obs`` (numpy) and ``save(path)`` / ``load_stats(path)``
(an ``.npz`` of the env's ``normalize_state()``; not SB3's pickle).  With pixel observations only ``agent_pos`` is
normalised, and nothing more is copied to the host than without the option.

``replay=dict(buffer_size=...)`` is forwarded to the env (GoalEnv, state observation): every ``step`` then stores its
transitions in the device-resident hindsight buffer, and ``SO100HerReplayBuffer`` below hands it to an
off-policy learner in ``HerReplayBuffer``'s place: ``add`` has nothing left to do, ``sample`` returns device tensors.

The image (or flattened) tensor reaches the host by one asynchronous copy into pinned memory and one stream
synchronisation per step.  Two pinned buffers alternate: **the image array of an observation returned by
``reset()`` / ``step()`` stays valid through the next ``step()`` and is overwritten by the one after it** (SB3's
collectors hold ``_last_obs`` across one step); copy it to keep it longer.
"""
import collections
import time

import numpy as np

from . import spaces
from .vec_env import SO100VecEnv

try:  # optional dependency (absent in this image)
    from stable_baselines3.common.vec_env.base_vec_env import VecEnv as _VecEnvBase
except ImportError:  # pragma: no cover - exercised when SB3 is installed
    _VecEnvBase = object
try:
    from stable_baselines3.common.buffers import ReplayBuffer as _ReplayBufferBase
except ImportError:  # pragma: no cover
    _ReplayBufferBase = object


def _np(t):
    return t.detach().cpu().numpy()


class SO100SB3VecEnv(_VecEnvBase):
    """N SO-ARM100 envs on one GPU behind SB3's VecEnv interface (numpy in / numpy out)."""

    metadata = {"render_modes": []}

    def __init__(self, num_envs, task="so100_cube_to_bin", device="cuda:0", seed=0, max_episode_steps=None,
                 domain_randomization=None, env_offset=0, iterations=None, solver="newton", obs_type="so100_state",
                 observation_width=640, observation_height=480, channels_first=False, cameras=None, shadows=False,
                 antialias=False, action_mode="joint", ee_control=None, normalize=None, replay=None,
                 uniform_replay=None):
        self.pixel_obs = obs_type == "so100_pixels_agent_pos"
        kw = {}
        self._last_obs = None                      # the observation last returned (get_original_obs: its image)
        if shadows and not self.pixel_obs:
            raise ValueError("shadows need obs_type='so100_pixels_agent_pos'")
        if antialias and not self.pixel_obs:
            raise ValueError("antialias needs obs_type='so100_pixels_agent_pos'")
        if cameras is not None:
            if not self.pixel_obs:
                raise ValueError("cameras need obs_type='so100_pixels_agent_pos'")
            if task != "so100_goal" and not channels_first:
                raise ValueError("cameras need channels_first=True: the K images are stacked along the channel axis, "
                                 "[3K,H,W]")
        if self.pixel_obs:
            kw = dict(obs_type=obs_type, observation_width=observation_width, observation_height=observation_height,
                      channels_first=channels_first, flat_pixels=task == "so100_goal")
            if cameras is not None:
                kw["cameras"] = cameras
            if shadows:
                kw["shadows"] = shadows
            if antialias:
                kw["antialias"] = antialias
        elif obs_type != "so100_state":
            raise NotImplementedError(f"obs_type={obs_type!r}: 'so100_state' or 'so100_pixels_agent_pos'")
        elif channels_first:
            raise ValueError("channels_first needs obs_type='so100_pixels_agent_pos'")
        if action_mode != "joint" or ee_control is not None:      # the env's own checks (ValueError) apply
            kw["action_mode"], kw["ee_control"] = action_mode, ee_control
        if normalize is not None:                                  # the env's own checks (ValueError) apply
            kw["normalize"] = normalize
        if replay is not None:                                     # the env's own checks (ValueError) apply
            kw["replay"] = replay
        if uniform_replay is not None:                             # the env's own checks (ValueError) apply
            kw["uniform_replay"] = uniform_replay
        self.venv = SO100VecEnv(num_envs, task=task, device=device, seed=seed, max_episode_steps=max_episode_steps,
                                autoreset=True, domain_randomization=domain_randomization, env_offset=env_offset,
                                iterations=iterations, solver=solver, episode_stats=True, **kw)
        self._t0 = time.time()
        n = self.venv.num_envs
        obs_box = spaces.Box(low=-np.inf, high=np.inf, shape=(15,), dtype=np.float32)
        goal_box = spaces.Box(low=-np.inf, high=np.inf, shape=(3,), dtype=np.float32)
        self._host = None
        if self.pixel_obs:
            import torch
            r = self.venv.renderer
            src = self.venv.pixels_flat if self.venv.is_goal else self.venv.pixels
            if cameras is not None and not self.venv.is_goal:
                src = src.view(n, -1, r.height, r.width)         # [N,K,3,H,W] as [N,3K,H,W]: no copy
            # the two pinned host buffers the image / flattened observation alternates between
            self._host = [torch.empty(src.shape, dtype=src.dtype, pin_memory=True) for _ in range(2)]
            self._host_i = 0
            if self.venv.is_goal:
                obs_space = spaces.Dict({
                    "observation": spaces.Box(low=-np.inf, high=np.inf, shape=(src.shape[1],), dtype=np.float32),
                    "achieved_goal": goal_box, "desired_goal": goal_box})
            else:
                obs_space = spaces.Dict({
                    "pixels": spaces.Box(low=0, high=255, shape=tuple(src.shape[1:]), dtype=np.uint8),
                    "agent_pos": spaces.Box(low=-10.0, high=10.0, shape=(6,), dtype=np.float32)})
        elif self.venv.is_goal:
            obs_space = spaces.Dict({
                "observation": obs_box,
                "achieved_goal": spaces.Box(low=-np.inf, high=np.inf, shape=(3,), dtype=np.float32),
                "desired_goal": spaces.Box(low=-np.inf, high=np.inf, shape=(3,), dtype=np.float32)})
        else:
            obs_space = obs_box
        act_space = spaces.Box(low=-1, high=1, shape=(self.venv.action_dim,), dtype=np.float32)
        if self.pixel_obs:
            self.metadata = {"render_modes": ["rgb_array"]}
            self.render_mode = "rgb_array"          # read back by SB3's VecEnv.__init__ through get_attr
        if _VecEnvBase is not object:
            super().__init__(n, obs_space, act_space)
        else:
            self.num_envs = n
            self.observation_space = obs_space
            self.action_space = act_space
            self.render_mode = "rgb_array" if self.pixel_obs else None
        self._next_seeds = None
        self._actions = None
        self.reset_infos = [{} for _ in range(n)]

    # ------------------------------------------------------------------ SB3 VecEnv API
    def seed(self, seed=None):
        """Seeds for the next reset(): env i <- seed + i (SB3 VecEnv.seed); None -> in-kernel seeds."""
        if seed is None:
            self._next_seeds = None
            return [None] * self.num_envs
        self._next_seeds = int(seed)
        return [int(seed) + i for i in range(self.num_envs)]

    def reset(self):
        seed, self._next_seeds = self._next_seeds, None
        obs, _ = self.venv.reset(seed=seed)
        self.reset_infos = [{} for _ in range(self.num_envs)]
        return self._obs_np(obs)

    def step_async(self, actions):
        a = np.asarray(actions, dtype=np.float32)
        k = self.venv.action_dim
        if a.shape != (self.num_envs, k):
            raise ValueError(f"actions must be [{self.num_envs}, {k}], got {a.shape}")
        self._actions = a

    def step_wait(self):
        if self._actions is None:
            raise RuntimeError("step_wait() without step_async()")
        v = self.venv
        prev_goal = v.desired_goal.clone() if v.is_goal else None   # the auto-reset resamples done envs' goals
        obs, rew, term, trunc, info = v.step(self._actions)
        self._actions = None
        done_t = term | trunc
        rewards = _np(rew).astype(np.float32)
        terminated, truncated = _np(term), _np(trunc)
        dones = terminated | truncated
        success = _np(info["is_success"])
        infos = [{"is_success": bool(success[i])} for i in range(self.num_envs)]
        idx = np.flatnonzero(dones)
        if idx.size:
            fachieved = None
            if v.final_obs_norm is None:
                final = _np(v.final_obs[done_t])
                if v.is_goal:
                    fgoal = _np(prev_goal[done_t])
            else:                                            # normalize: the finished rows, normalised on the device
                final = _np(v.final_obs_norm[done_t])        # (pixel observations: [.,6], agent_pos alone)
                if v.is_goal:
                    g = v.normalize_obs({"achieved_goal": v.final_obs[done_t][:, 0:3], "desired_goal": prev_goal[done_t]})
                    fachieved, fgoal = _np(g["achieved_goal"]), _np(g["desired_goal"])
            if self.pixel_obs:
                fpix = _np(v.final_pixels[done_t])           # only the done envs' images, gathered on the device
                if v.camera_names is not None and not v.is_goal:
                    fpix = fpix.reshape(idx.size, *self._host[0].shape[1:])      # [K,3,H,W] as [3K,H,W]
                if v.is_goal:                                # _flatten_observation (env.py:267-270), in numpy
                    fflat = np.concatenate([fpix.reshape(idx.size, -1).astype(np.float32) / np.float32(255.0),
                                            final[:, 9:15]], axis=1)
            for k, i in enumerate(idx):
                if self.pixel_obs and v.is_goal:
                    term_obs = {"observation": fflat[k], "achieved_goal": final[k, 0:3].copy(),
                                "desired_goal": fgoal[k]}
                elif self.pixel_obs:
                    term_obs = {"pixels": fpix[k],
                                "agent_pos": (final[k, 9:15] if v.final_obs_norm is None else final[k]).copy()}
                elif v.is_goal:
                    term_obs = {"observation": final[k],
                                "achieved_goal": final[k, 0:3].copy() if fachieved is None else fachieved[k],
                                "desired_goal": fgoal[k]}
                else:
                    term_obs = final[k]
                infos[i]["terminal_observation"] = term_obs
                infos[i]["TimeLimit.truncated"] = bool(truncated[i] and not terminated[i])
            # VecMonitor's info["episode"], from the kernel's episode statistics (return in float64, as the
            # reference's rewards)
            ep = _np(v.ep_final[done_t])
            t = round(time.time() - self._t0, 6)
            for k, i in enumerate(idx):
                infos[i]["episode"] = {"r": float(ep[k, 0]), "l": int(ep[k, 1]), "t": t}
        return self._obs_np(obs), rewards, dones, infos

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    def close(self):
        self.venv.close()

    def get_images(self):
        """Pixel observations: the N current camera images as [H,W,3] uint8 arrays (transposing views of the host
        copy when the env stores them channel-first).  State observations draw no camera: N times None."""
        if not self.pixel_obs:
            return [None] * self.num_envs
        img = _np(self.venv.pixels)
        if self.venv.camera_names is not None:               # several cameras: the first one's images
            img = img[:, 0]
        if self.venv.channels_first:
            img = img.transpose(0, 2, 3, 1)
        return [img[i] for i in range(self.num_envs)]

    def render(self, mode=None):
        """Pixel observations: the current images, tiled by SB3's own ``VecEnv.render`` when SB3 is importable,
        else stacked [N,H,W,3].  State observations: None."""
        if not self.pixel_obs:
            return None
        if _VecEnvBase is not object:
            return super().render(mode)
        return np.stack(self.get_images())

    def _indices(self, indices):
        if indices is None:
            return list(range(self.num_envs))
        if isinstance(indices, (int, np.integer)):
            return [int(indices)]
        return [int(i) for i in indices]

    def get_attr(self, attr_name, indices=None):
        val = getattr(self.venv, attr_name) if hasattr(self.venv, attr_name) else getattr(self, attr_name)
        return [val for _ in self._indices(indices)]

    def set_attr(self, attr_name, value, indices=None):
        if hasattr(self.venv, attr_name):
            raise AttributeError(f"{attr_name!r} is shared by all envs of the batch and cannot be set per env")
        setattr(self, attr_name, value)

    def env_method(self, method_name, *method_args, indices=None, **method_kwargs):
        idx = self._indices(indices)
        if method_name == "compute_reward":
            # HerReplayBuffer: one batched call for the first index, answered on the device
            achieved, desired = method_args[0], method_args[1]
            r = _np(self.venv.compute_reward(achieved, desired))
            shape = np.shape(achieved)[:-1]
            return [r.reshape(shape)] + [None] * (len(idx) - 1)
        fn = getattr(self.venv, method_name)
        out = fn(*method_args, **method_kwargs)
        return [out for _ in idx]

    def env_is_wrapped(self, wrapper_class, indices=None):
        return [False for _ in self._indices(indices)]

    # ------------------------------------------------------------------ VecNormalize's surface (normalize=...)
    @property
    def obs_rms(self):
        """key -> .mean / .var / .count (the state env's single key: that object itself, as VecNormalize's obs_rms)"""
        rms = self.venv.obs_rms
        return rms["obs"] if set(rms) == {"obs"} else rms

    @obs_rms.setter
    def obs_rms(self, rms):
        self.venv.obs_rms = rms

    @property
    def ret_rms(self):
        return self.venv.ret_rms

    @ret_rms.setter
    def ret_rms(self, rms):
        self.venv.ret_rms = rms

    @property
    def training(self):
        return self.venv.training

    @training.setter
    def training(self, on):
        self.venv.training = on

    @property
    def norm_obs(self):
        return self.venv.obs_norm is not None or self.venv.agent_pos_norm is not None

    @property
    def norm_reward(self):
        return self.venv.reward_norm is not None

    def get_original_obs(self):
        """The raw observation behind the last one returned (read from the device now: valid until the next step)."""
        v = self.venv
        v._normalizer()
        if self.pixel_obs:
            out = dict(self._last_obs)
            out["agent_pos"] = _np(v.obs[:, 9:15])
            return out
        if v.is_goal:
            return {"observation": _np(v.obs), "achieved_goal": _np(v.achieved_goal), "desired_goal": _np(v.desired_goal)}
        return _np(v.obs)

    def get_original_reward(self):
        """The raw rewards of the last step."""
        self.venv._normalizer()
        return _np(self.venv.reward).astype(np.float32)

    def _to_device(self, obs):
        import torch
        if isinstance(obs, dict):
            return {k: (torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32, device=self.venv.device)
                        if k in self.venv._normalizer().cols else x) for k, x in obs.items()}
        return torch.as_tensor(np.ascontiguousarray(obs), dtype=torch.float32, device=self.venv.device)

    def _to_host(self, obs):
        if isinstance(obs, dict):
            return {k: (_np(x) if hasattr(x, "detach") else x) for k, x in obs.items()}
        return _np(obs)

    def normalize_obs(self, obs):
        """numpy (or a dict of numpy) -> the normalised observation, by the device kernel, with the current statistics"""
        return self._to_host(self.venv.normalize_obs(self._to_device(obs)))

    def unnormalize_obs(self, obs):
        return self._to_host(self.venv.unnormalize_obs(self._to_device(obs)))

    def save(self, path):
        """The statistics and options as an ``.npz`` (``normalize_state()``), bit for bit."""
        with open(path, "wb") as f:
            np.savez(f, **self.venv.normalize_state())

    def load_stats(self, path):
        """Take the statistics ``save`` wrote (the options stay this env's)."""
        with np.load(path) as z:
            self.venv.set_normalize_state({k: z[k] for k in z.files})

    # ------------------------------------------------------------------ helpers
    def _obs_np(self, obs):
        out = self._obs_np_inner(obs)
        if self.venv._norm is not None:            # (get_original_obs hands the image of this observation back)
            self._last_obs = out
        return out

    def _obs_np_inner(self, obs):
        if self._host is not None:
            # the large tensor: one asynchronous copy into the pinned buffer of this step, one synchronisation
            import torch
            big = "observation" if self.venv.is_goal else "pixels"
            host = self._host[self._host_i]
            self._host_i ^= 1
            host.copy_(obs[big].view(host.shape), non_blocking=True)
            out = {k: _np(t) for k, t in obs.items() if k != big}
            torch.cuda.current_stream(self.venv.device).synchronize()
            out[big] = host.numpy()
            return out
        if isinstance(obs, dict):
            return {k: _np(t) for k, t in obs.items()}
        return _np(obs)

    @property
    def unwrapped(self):
        return self

    @property
    def device(self):
        return self.venv.device


# SB3's DictReplayBufferSamples, field for field (type_aliases.py); the values are device tensors
HerReplaySamples = collections.namedtuple("HerReplaySamples",
                                          ["observations", "actions", "next_observations", "dones", "rewards"])


class SO100HerReplayBuffer(_ReplayBufferBase):
    """The env's device-resident hindsight buffer (``SO100VecEnv(replay=...)``) behind the calls an
    SB3 off-policy learner makes on ``HerReplayBuffer``: ``SAC(..., replay_buffer_class=SO100HerReplayBuffer,
    replay_buffer_kwargs=dict(env=env))``.  The env has stored every transition by the time the learner calls ``add``, so
    ``add`` does nothing; ``sample`` draws and relabels on the device and returns torch tensors there.  SB3's own storage
    is never allocated (its ``__init__`` is not run)."""

    def __init__(self, buffer_size=None, observation_space=None, action_space=None, env=None, device="auto", n_envs=None,
                 **_ignored):
        venv = getattr(env, "venv", env)
        if venv is None or getattr(venv, "replay", None) is None:
            raise ValueError("SO100HerReplayBuffer needs env=: an SO100SB3VecEnv / SO100VecEnv built with replay=...")
        self.venv, self.replay = venv, venv.replay
        self.buffer_size = self.replay.T                     # SB3 counts slots per env
        self.n_envs = venv.num_envs
        self.observation_space = observation_space if observation_space is not None else \
            getattr(env, "observation_space", None)
        self.action_space = action_space if action_space is not None else getattr(env, "action_space", None)
        self.device = venv.device
        self.pos, self.full = 0, False

    def add(self, *args, **kwargs):
        """nothing: ``step`` has already pushed this transition on the device"""

    def size(self):
        """the transitions a sample draws from (waits for the device)"""
        return self.replay.size()

    def sample(self, batch_size, env=None):
        """observations / next_observations: dicts of [B, .] tensors (observation, achieved_goal, desired_goal), normalised
        where the env was built with ``normalize=...``; actions [B, A]; dones and rewards [B, 1]."""
        b = self.replay.sample(batch_size, normalize=self.venv._norm is not None)
        keys = ("observation", "achieved_goal", "desired_goal")
        return HerReplaySamples(observations={k: b[k] for k in keys}, actions=b["actions"],
                                next_observations={k: b["next_" + k] for k in keys},
                                dones=b["dones"].reshape(-1, 1), rewards=b["rewards"].reshape(-1, 1))


# SB3's ReplayBufferSamples / DictReplayBufferSamples, field for field (type_aliases.py); the values are device tensors
ReplaySamples = collections.namedtuple("ReplaySamples",
                                       ["observations", "actions", "next_observations", "dones", "rewards"])
# the same five and the factor of the bootstrap value, gamma^m, for a buffer built with n_step: what a learner with
# n-step targets reads from its samples
NStepReplaySamples = collections.namedtuple("NStepReplaySamples", ReplaySamples._fields + ("discounts",))
# a buffer built with prioritized: the importance weights [B, 1] (divided by the batch's greatest) and what
# update_priorities takes back, after the fields above
_PER_FIELDS = ("weights", "env_indices", "slot_indices")
PrioritizedReplaySamples = collections.namedtuple("PrioritizedReplaySamples", ReplaySamples._fields + _PER_FIELDS)
PrioritizedNStepReplaySamples = collections.namedtuple("PrioritizedNStepReplaySamples",
                                                       NStepReplaySamples._fields + _PER_FIELDS)


class SO100ReplayBuffer(_ReplayBufferBase):
    """The env's device-resident uniform buffer (``SO100VecEnv(uniform_replay=...)``) behind the calls
    an SB3 off-policy learner makes on ``ReplayBuffer`` / ``DictReplayBuffer``: ``SAC(...,
    replay_buffer_class=SO100ReplayBuffer, replay_buffer_kwargs=dict(env=env))``.  The env has stored every transition by
    the time the learner calls ``add``, so ``add`` does nothing; ``sample`` draws (and, with ``augment``, shifts the
    images) on the device and returns torch tensors there.  SB3's own storage is never allocated (its ``__init__`` is
    not run).  ``n_steps`` and ``gamma``, which a learner with n-step targets passes to its buffer, are ignored for an
    env built without ``uniform_replay=dict(n_step=...)``; with it they must agree with the env's options (ValueError
    otherwise), and ``sample`` returns ``NStepReplaySamples``: the five fields and ``discounts`` [B, 1].  For an env built
    with ``uniform_replay=dict(prioritized=...)`` the samples also carry ``weights`` [B, 1],
    ``env_indices`` and ``slot_indices`` [B], and ``update_priorities`` takes the two index fields back with |TD error|.
    Nothing is claimed about SB3's own classes: a learner that uses these fields reads them by name."""

    def __init__(self, buffer_size=None, observation_space=None, action_space=None, env=None, device="auto", n_envs=None,
                 n_steps=None, gamma=None, **_ignored):
        venv = getattr(env, "venv", env)
        if venv is None or getattr(venv, "uniform_replay", None) is None:
            raise ValueError("SO100ReplayBuffer needs env=: an SO100SB3VecEnv / SO100VecEnv built with "
                             "uniform_replay=...")
        self.venv, self.replay = venv, venv.uniform_replay
        if self.replay.n_step is not None:
            if n_steps is not None and int(n_steps) != self.replay.n_step:
                raise ValueError(f"SO100ReplayBuffer: n_steps {n_steps} but the env was built with uniform_replay="
                                 f"dict(n_step={self.replay.n_step})")
            if gamma is not None and float(gamma) != self.replay.gamma:
                raise ValueError(f"SO100ReplayBuffer: gamma {gamma} but the env was built with uniform_replay="
                                 f"dict(gamma={self.replay.gamma})")
        self.buffer_size = self.replay.T                     # SB3 counts slots per env
        self.n_envs = venv.num_envs
        self.observation_space = observation_space if observation_space is not None else \
            getattr(env, "observation_space", None)
        self.action_space = action_space if action_space is not None else getattr(env, "action_space", None)
        self.device = venv.device
        self.pos, self.full = 0, False

    def add(self, *args, **kwargs):
        """nothing: ``step`` has already pushed this transition on the device"""

    def size(self):
        """the transitions a sample draws from (waits for the device)"""
        return self.replay.size()

    def sample(self, batch_size, env=None):
        """observations / next_observations: the dict {"pixels" [B, ...] uint8, "agent_pos" [B, 6]} of a pixel env, the
        [B, 15] tensor of a state env, the float part normalised where the env was built with ``normalize=dict(obs=True,
        ...)``; actions [B, A]; dones and rewards [B, 1]."""
        norm = self.venv._norm
        b = self.replay.sample(batch_size, normalize=norm is not None and bool(norm.out))
        if "pixels" in b:
            obs = {"pixels": b["pixels"], "agent_pos": b["agent_pos"]}
            nxt = {"pixels": b["next_pixels"], "agent_pos": b["next_agent_pos"]}
        else:
            obs, nxt = b["obs"], b["next_obs"]
        if "weights" in b:
            more = dict(weights=b["weights"].reshape(-1, 1), env_indices=b["env"], slot_indices=b["slot"])
            if "discounts" in b:
                return PrioritizedNStepReplaySamples(observations=obs, actions=b["actions"], next_observations=nxt,
                                                     dones=b["dones"].reshape(-1, 1),
                                                     rewards=b["rewards"].reshape(-1, 1),
                                                     discounts=b["discounts"].reshape(-1, 1), **more)
            return PrioritizedReplaySamples(observations=obs, actions=b["actions"], next_observations=nxt,
                                            dones=b["dones"].reshape(-1, 1), rewards=b["rewards"].reshape(-1, 1), **more)
        if "discounts" in b:
            return NStepReplaySamples(observations=obs, actions=b["actions"], next_observations=nxt,
                                      dones=b["dones"].reshape(-1, 1), rewards=b["rewards"].reshape(-1, 1),
                                      discounts=b["discounts"].reshape(-1, 1))
        return ReplaySamples(observations=obs, actions=b["actions"], next_observations=nxt,
                             dones=b["dones"].reshape(-1, 1), rewards=b["rewards"].reshape(-1, 1))

    def update_priorities(self, env_indices, slot_indices, td_abs):
        """|TD error| of a sampled batch back into the priorities (``UniformReplay.update_priorities``); ValueError for an
        env built without ``uniform_replay=dict(prioritized=...)``"""
        self.replay.update_priorities(env_indices, slot_indices, td_abs)
