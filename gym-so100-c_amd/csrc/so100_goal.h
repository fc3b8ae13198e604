// so100_goal.h - the GoalEnv's sparse reward (env.py:341-353) as one device function: so100_goal_reward
// (so100_step.hip) and the hindsight relabelling of so100_her_sample (so100_her.hip) call the same arithmetic.
#pragma once
#include <hip/hip_runtime.h>

namespace so100 {

// np.linalg.norm(achieved - desired) in float32 (env.py:347-349): 0 inside the threshold, else -1
__device__ __forceinline__ float goal_reward_f32(float a0, float a1, float a2, float g0, float g1, float g2,
                                                 float threshold) {
  float d0 = a0 - g0, d1 = a1 - g1, d2 = a2 - g2;
  float dist = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
  return dist < threshold ? 0.f : -1.f;
}

}  // namespace so100
