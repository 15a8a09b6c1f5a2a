// tools/custom_env_timing.py: SynthReach-v0's description through the generic per-step kernel at 16, 32 and 64 lanes
// per env.  OBS = 60 makes the row the one the built-in env writes (6 native columns, zeros to 60), so that the figures
// compare kernels and not row widths; Reach6 is the description as it stands (6 columns).
#pragma once
struct ReachWide : OsaReachEnv {
  static constexpr int OBS = 60;
};
struct ReachWide16 : ReachWide {
  static constexpr int LANES = 16;
};
struct ReachWide32 : ReachWide {
  static constexpr int LANES = 32;
};
struct ReachWide64 : ReachWide {
  static constexpr int LANES = 64;
};
using Reach6 = OsaReachEnv;
