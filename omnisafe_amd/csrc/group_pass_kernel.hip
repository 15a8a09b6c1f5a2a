// GROUPED PERSISTENT PASS: the plain pass of ppo_pass_body.h for n independent agents in ONE launch.
//
// Replaces the reference's way of running the seeds and hyper-parameter variants of an experiment:
// ExperimentGrid.run (omnisafe/common/experiment_grid.py:387-471) hands every variant to a process pool, one
// training per worker process.  One agent's pass occupies 3 compute units (one workgroup per network, weights in LDS,
// Adam moments in registers) for ~9 us per 64-row step; the workgroups never wait for each other, so the passes of n
// agents are simply 3 n workgroups of one grid.  Workgroup (member s, network k) runs osa_ppo_pass_body on member s's
// own argument block -- the same body, the same operands, the same bits as n calls of osa_ppo_pass_ext.
//
// The members' argument blocks (OsaPassArgs, a few hundred bytes each) do not fit the launch arguments, so they are
// STAGED in the caller's device workspace by small copy launches that carry them as launch arguments: the runtime
// takes its copy of launch arguments before a launch call returns, and the stream orders the copy launches behind
// the previous grouped pass -- so neither the host blocks nor the workspace can be overwritten while an earlier
// launch still needs them, with no host synchronisation and no event.
#include "ppo_pass_body.h"

#include <vector>

struct OsaGroupArgs {
  const OsaPassArgs* members;  // [n] staged argument blocks (device)
  int n;
};

// argument blocks per staging launch (launch arguments are limited to 4 KB)
constexpr int OSA_STAGE_N = (int)((3584 - 16) / sizeof(OsaPassArgs));
static_assert(OSA_STAGE_N >= 1 && sizeof(OsaPassArgs) % sizeof(int) == 0, "staging copies whole words");
struct OsaStageArgs {
  OsaPassArgs m[OSA_STAGE_N];
  OsaPassArgs* dst;
  int count;
};

__global__ __launch_bounds__(256) void osa_group_stage_kernel(OsaStageArgs s) {
  constexpr int W = (int)(sizeof(OsaPassArgs) / sizeof(int));
  const int* src = reinterpret_cast<const int*>(s.m);
  int* dst = reinterpret_cast<int*>(s.dst);
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < s.count * W; e += gridDim.x * blockDim.x) dst[e] = src[e];
}

// A pointer that arrives as a launch argument is known to point to global memory; one read from a staged block is a
// generic pointer, and every access through it a FLAT instruction, which counts against the LDS counter as well and
// so serialises with the body's LDS traffic (measured: 9.7 instead of 8.9 us per 64-row step).  The round trip
// through the global address space tells the compiler what the launch-argument form knows; the empty asm keeps the two
// casts from being folded away.  No instruction is emitted.
template <class T>
__device__ __forceinline__ T* osa_global(T* p) {
  __attribute__((address_space(1))) T* g = (__attribute__((address_space(1))) T*)p;
  asm volatile("" : "+s"(g));
  return (T*)g;
}

// Grid 24 ceil(n / 8): member s, network k is block 8 (3 (s / 8) + k) + s % 8.  Blocks b and b + 8 share an XCC, so a
// member's three workgroups share one (its rows come from HBM once, as with one_xcc of the solo launch) and the
// members spread over the eight XCCs.  Placement is for speed only: no workgroup waits for another.
template <int KB, int OT, bool MULTI, bool EXT, bool SO>
__global__ __launch_bounds__(256, 1) void osa_ppo_pass_group_kernel(OsaGroupArgs g) {
  const int q = blockIdx.x >> 3;
  const int s = 8 * (q / 3) + (blockIdx.x & 7), net = q % 3;
  if (s >= g.n) return;
  OsaPassArgs a = g.members[s];  // (uniform address, nothing stored before: scalar loads into SGPRs)
  a.params = osa_global(a.params); a.adam_m = osa_global(a.adam_m); a.adam_v = osa_global(a.adam_v);
  a.adam_step = osa_global(a.adam_step); a.obs = osa_global(a.obs); a.act = osa_global(a.act);
  a.logp = osa_global(a.logp); a.tgt_r = osa_global(a.tgt_r); a.tgt_c = osa_global(a.tgt_c);
  a.adv_r = osa_global(a.adv_r); a.adv_c = osa_global(a.adv_c); a.perm = osa_global(a.perm);
  a.lagrange = osa_global(a.lagrange); a.stats = osa_global(a.stats); a.old_mean = osa_global(a.old_mean);
  a.old_log_std = osa_global(a.old_log_std);
  if (!((a.nets_mask >> net) & 1)) return;
  osa_ppo_pass_body<KB, OT, MULTI, false, EXT, false, false, SO>(a, net, 0);
}

template <int KB, int OT, bool MULTI, bool EXT>
static int osa_launch_group(const OsaGroupArgs& g, const OsaNet& nd, hipStream_t stream) {
  const dim3 grid(24 * ((g.n + 7) / 8));
  return osa_pass_so<OT>(nd, [&](auto SO) {
    return osa_launch_pass_kernel<osa_ppo_pass_group_kernel<KB, OT, MULTI, EXT, SO>>(g, nd, grid, stream);
  });
}

extern "C" {

size_t osa_ppo_pass_group_ws_bytes(int n) { return n > 0 ? (size_t)n * sizeof(OsaPassArgs) : 0; }

int osa_ppo_pass_group(int obs_dim, int act_dim, int hidden, const osa_pass_member* members, int n, void* workspace,
                       size_t workspace_bytes, void* stream) {
  if (!osa_ppo_pass_supported(obs_dim, act_dim, hidden)) return OSA_EUNSUPPORTED;
  OSA_REQUIRE(members && n >= 1 && workspace && workspace_bytes >= osa_ppo_pass_group_ws_bytes(n));
  OSA_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0);
  // every member checked and its class known before anything is enqueued
  std::vector<OsaPassArgs> args((size_t)n);
  bool multi = false, extended = false;
  for (int s = 0; s < n; ++s) {
    const osa_pass_member& m = members[s];
    bool ext_s = false;
    const int rc = osa_plain_pass_args(args[s], &ext_s, obs_dim, act_dim, hidden, m.params, m.adam_m, m.adam_v,
                                       m.adam_step, m.obs, m.ld_obs, m.act, m.ld_act, m.logp, m.target_value_r,
                                       m.target_value_c, m.adv_r, m.adv_c, m.perm, m.M, m.B, m.lagrange, &m.hp,
                                       m.loss_kind, m.nets_mask, m.step_stats, m.has_ext ? &m.ext : nullptr);
    if (rc != OSA_OK) return rc;
    const bool multi_s = m.B > 64;
    if (s == 0) {
      multi = multi_s;
      extended = ext_s;
    } else if (multi_s != multi || ext_s != extended) {
      return OSA_EINVAL;  // one template instantiation per launch: the caller sorts its members by class
    }
  }
  hipStream_t st = osa_stream(stream);
  OsaPassArgs* dev = static_cast<OsaPassArgs*>(workspace);
  for (int s0 = 0; s0 < n; s0 += OSA_STAGE_N) {
    OsaStageArgs sa;
    sa.count = n - s0 < OSA_STAGE_N ? n - s0 : OSA_STAGE_N;
    sa.dst = dev + s0;
    for (int k = 0; k < sa.count; ++k) sa.m[k] = args[(size_t)s0 + k];
    for (int k = sa.count; k < OSA_STAGE_N; ++k) sa.m[k] = OsaPassArgs{};
    hipLaunchKernelGGL(osa_group_stage_kernel, dim3(1), dim3(256), 0, st, sa);
    OSA_CHECK_LAUNCH();
  }
  const OsaGroupArgs g = {dev, n};
  const OsaNet& nd = args[0].nd;
  return osa_pass_shapes(nd.KB, nd.OUTP / 16, [&](auto K, auto O) {
    if (extended) return osa_launch_group<K, O, false, true>(g, nd, st);
    return multi ? osa_launch_group<K, O, true, false>(g, nd, st) : osa_launch_group<K, O, false, false>(g, nd, st);
  });
}

}  // extern "C"
