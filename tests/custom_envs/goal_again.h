// The built-in Goal descriptions, re-declared out of tree: OsaNavEnv<robot, OsaGoal> has LDS_ROW = true and the
// fresh_obj the contract asks for, so it is a valid custom description as it stands, and the generic row kernel must
// give the bits of osa_nav_env_step / osa_car_goal_env_step.  The numbered structs state the lanes per env.
#pragma once
struct GoalAgain : OsaPointGoal {};
struct CarGoalAgain : OsaCarGoal {};
#define GOAL_AGAIN_LANES(L)                \
  struct GoalAgain##L : OsaPointGoal {     \
    static constexpr int LANES = L;        \
  };                                       \
  struct CarGoalAgain##L : OsaCarGoal {    \
    static constexpr int LANES = L;        \
  }
GOAL_AGAIN_LANES(16);
GOAL_AGAIN_LANES(32);
GOAL_AGAIN_LANES(64);
#undef GOAL_AGAIN_LANES
