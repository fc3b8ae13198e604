"""The SB3 adapter with the reference's training observation, obs_type="so100_pixels_agent_pos" (gym_so100/sb3.py;
reference scripts/train_sac.py:294-310, env.py:50-66 and 219-238): spaces, both image layouts, SB3's auto-reset
contract with image observations, the two alternating pinned host buffers, the GoalEnv's flattened observation and
get_images().  As in test_gpu_sb3.py a pixel SO100VecEnv that is never reset runs the same episodes as reference.
Every comparison is bitwise."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

W, H = 40, 30
TABLE = np.arange(256, dtype=np.float32) / np.float32(255)       # env.py:267-270: astype(np.float32) / 255.0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def hwc(img, channels_first):
    """[..., H, W, 3] view of an image (batch) in either layout"""
    return np.moveaxis(img, -3, -1) if channels_first else img


@pytest.mark.parametrize("channels_first", [False, True])
def test_sb3_pixel_observation_and_terminal_observation(channels_first):
    from gym_so100 import SO100VecEnv
    from gym_so100.sb3 import SO100SB3VecEnv
    n, limit = 12, 4
    px = dict(obs_type="so100_pixels_agent_pos", observation_width=W, observation_height=H)
    env = SO100SB3VecEnv(n, seed=3, max_episode_steps=limit, channels_first=channels_first, **px)
    ref = SO100VecEnv(n, seed=3, max_episode_steps=0, autoreset=False, **px)     # same episodes, never reset
    shape = (3, H, W) if channels_first else (H, W, 3)
    sp = env.observation_space
    assert set(sp.spaces) == {"pixels", "agent_pos"}
    assert sp["pixels"].shape == shape and sp["pixels"].dtype == np.uint8
    assert int(sp["pixels"].low.min()) == 0 and int(sp["pixels"].high.max()) == 255
    assert sp["agent_pos"].shape == (6,) and sp["agent_pos"].dtype == np.float32
    assert float(sp["agent_pos"].low.min()) == -10.0 and float(sp["agent_pos"].high.max()) == 10.0
    env.seed(7)
    obs = env.reset()
    r_obs, _ = ref.reset(seed=7)
    assert set(obs) == {"pixels", "agent_pos"}
    assert isinstance(obs["pixels"], np.ndarray) and obs["pixels"].shape == (n,) + shape
    assert obs["pixels"].dtype == np.uint8 and obs["pixels"].any()
    assert obs["agent_pos"].shape == (n, 6) and obs["agent_pos"].dtype == np.float32
    np.testing.assert_array_equal(hwc(obs["pixels"], channels_first), r_obs["pixels"].cpu().numpy())
    np.testing.assert_array_equal(obs["agent_pos"], r_obs["agent_pos"].cpu().numpy())
    rng = np.random.default_rng(0)
    for t in range(limit):
        a = rng.uniform(-1, 1, size=(n, 6)).astype(np.float32)
        obs, rew, dones, infos = env.step(a)
        r_obs, r_rew, r_term, _, _ = ref.step(torch.from_numpy(a))
        r_pix, r_pos, r_term = r_obs["pixels"].cpu().numpy(), r_obs["agent_pos"].cpu().numpy(), r_term.cpu().numpy()
        np.testing.assert_array_equal(rew, r_rew.cpu().numpy())
        assert obs["pixels"].shape == (n,) + shape and obs["pixels"].dtype == np.uint8
        for i in range(n):
            assert "is_success" in infos[i]
            if dones[i]:
                term = infos[i]["terminal_observation"]
                assert set(term) == {"pixels", "agent_pos"}
                assert term["pixels"].shape == shape and term["pixels"].dtype == np.uint8
                np.testing.assert_array_equal(hwc(term["pixels"], channels_first), r_pix[i])
                np.testing.assert_array_equal(term["agent_pos"], r_pos[i])
                assert infos[i]["TimeLimit.truncated"] == (t == limit - 1 and not r_term[i])
            else:
                assert "terminal_observation" not in infos[i]
        live = ~dones
        np.testing.assert_array_equal(hwc(obs["pixels"], channels_first)[live], r_pix[live])
        np.testing.assert_array_equal(obs["agent_pos"][live], r_pos[live])
    assert dones.all()                                   # TimeLimit: every episode ended at step `limit`
    # the returned images are fresh episodes, not the terminal ones
    assert not np.array_equal(hwc(obs["pixels"], channels_first), r_pix)
    env.close()
    ref.close()


def test_observation_stays_valid_through_the_next_step():
    from gym_so100.sb3 import SO100SB3VecEnv
    n = 12
    env = SO100SB3VecEnv(n, seed=1, max_episode_steps=4, obs_type="so100_pixels_agent_pos", observation_width=W,
                         observation_height=H)
    rng = np.random.default_rng(1)
    prev = env.reset()
    kept = {k: v.copy() for k, v in prev.items()}
    for t in range(5):
        obs, _, _, _ = env.step(rng.uniform(-1, 1, size=(n, 6)).astype(np.float32))
        # the observation of the call before is still what it was; the new one is another array
        for k in kept:
            np.testing.assert_array_equal(prev[k], kept[k])
        assert not np.shares_memory(obs["pixels"], prev["pixels"])
        assert not np.array_equal(obs["pixels"], prev["pixels"])
        prev, kept = obs, {k: v.copy() for k, v in obs.items()}
    env.close()


def test_sb3_goal_env_flat_pixel_observation():
    from gym_so100.sb3 import SO100SB3VecEnv
    n, w, h = 8, 16, 12
    npix = 3 * w * h
    with pytest.raises(ValueError):
        SO100SB3VecEnv(n, task="so100_goal", obs_type="so100_pixels_agent_pos", observation_width=w,
                       observation_height=h, channels_first=True)
    env = SO100SB3VecEnv(n, task="so100_goal", seed=5, max_episode_steps=3, obs_type="so100_pixels_agent_pos",
                         observation_width=w, observation_height=h)
    sp = env.observation_space
    assert set(sp.spaces) == {"observation", "achieved_goal", "desired_goal"}
    assert sp["observation"].shape == (582,) and sp["observation"].dtype == np.float32
    obs = env.reset()
    assert obs["observation"].shape == (n, 582) and obs["observation"].dtype == np.float32
    assert obs["desired_goal"].shape == (n, 3) and obs["achieved_goal"].shape == (n, 3)
    img = np.stack(env.get_images())
    assert img.shape == (n, h, w, 3) and img.any()
    np.testing.assert_array_equal(bits(obs["observation"][:, :npix]), bits(TABLE[img.reshape(n, -1)]))
    np.testing.assert_array_equal(obs["observation"][:, npix:], env.venv.obs[:, 9:15].cpu().numpy())
    # HER relabelling: batched compute_reward through env_method (env.py:341-353)
    ach = obs["achieved_goal"]
    r = env.env_method("compute_reward", ach, obs["desired_goal"], [{}] * n, indices=[0])[0]
    d = np.linalg.norm(ach - obs["desired_goal"], axis=-1)
    np.testing.assert_array_equal(r, np.where(d < 0.01, 0.0, -1.0).astype(np.float32))
    assert np.all(env.env_method("compute_reward", ach, ach, [{}] * n, indices=[0])[0] == 0.0)
    goals = obs["desired_goal"].copy()
    for t in range(3):
        obs, rew, dones, infos = env.step(np.zeros((n, 6), np.float32))
        assert obs["observation"].shape == (n, 582)
    assert dones.all()
    fpix = env.venv.final_pixels.cpu().numpy()                  # the finished episodes' last images [n,h,w,3]
    fobs = env.venv.final_obs.cpu().numpy()
    assert fpix.any()
    for i in range(n):
        term = infos[i]["terminal_observation"]
        assert set(term) == {"observation", "achieved_goal", "desired_goal"}
        assert term["observation"].shape == (582,) and term["observation"].dtype == np.float32
        want = np.concatenate([fpix[i].reshape(-1).astype(np.float32) / np.float32(255.0), fobs[i, 9:15]])
        np.testing.assert_array_equal(bits(term["observation"]), bits(want))
        np.testing.assert_array_equal(term["desired_goal"], goals[i])       # the finished episode's goal
        np.testing.assert_array_equal(term["achieved_goal"], fobs[i, 0:3])
    env.close()


@pytest.mark.parametrize("channels_first", [False, True])
def test_get_images(channels_first):
    from gym_so100.sb3 import SO100SB3VecEnv
    n = 5
    env = SO100SB3VecEnv(n, seed=2, obs_type="so100_pixels_agent_pos", observation_width=W, observation_height=H,
                         channels_first=channels_first)
    env.reset()
    obs, _, _, _ = env.step(np.full((n, 6), 0.3, np.float32))
    imgs = env.get_images()
    assert len(imgs) == n
    for i in range(n):
        assert imgs[i].shape == (H, W, 3) and imgs[i].dtype == np.uint8
        np.testing.assert_array_equal(imgs[i], hwc(obs["pixels"][i], channels_first))
    frame = env.render()
    if type(env).__mro__[1] is object:                   # the duck-typed class: the images stacked
        np.testing.assert_array_equal(frame, np.stack(imgs))
    # the default observation draws no camera
    st = SO100SB3VecEnv(2)
    assert st.get_images() == [None, None] and st.render() is None
    st.close()
    env.close()
