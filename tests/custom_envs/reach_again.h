// SynthReach-v0's description through the generic per-step kernel, unchanged.
#pragma once
using ReachAgain = OsaReachEnv;
