// Off-policy TD3 and DDPG trained on the device from a replay ring: replaces omnisafe/algorithms/off_policy/
// ddpg.py:382-547 and td3.py:50-116, the ring of common/buffer/vector_offpolicy_buffer.py and MLPActor.predict.
//
// At the YAML defaults every env step is followed by one gradient step over 256 rows through seven small MLPs, each
// three dependent layers: the family is bound by launches, not by arithmetic.  td3_forward_kernel runs the whole
// forward of a step in ONE plain launch:
//   * a workgroup of four waves owns 32 rows of the batch and carries them through five networks (TD3: target actor,
//     two target critics, two online critics; with use_cost the online actor, the cost target and the cost critic too);
//     the activations never leave the chip: two ping-pong LDS buffers [32][256 + 4], one LDS array [32][obs || act]
//     that first holds next_obs || a' -- the action columns written by the actor's head -- and is then refilled with
//     obs || act of the same ring rows;
//   * rows come straight from the ring through idx[slot][row]: no gather launch;
//   * weights skip LDS (chain_layer.h: every wave owns output columns, one 16-byte global load feeds four float32
//     32x32x2 MFMAs); the heads (action, q) split K over the waves and meet in LDS in wave order;
//   * bias, activation, tanh, the clipped target-policy noise, the clamp, the min over the target pair, the TD target
//     and the TD error are fused into the accumulator write-backs; the online critics' layer outputs are written once to
//     the workspace on their way through, for the per-layer backward launches (crr_layers.h);
//   * no cooperative groups, no spin-waits, no atomics; the losses are reduced in a fixed order by the Adam launch.
// The layer route (OSA_TD3_ROUTE_LAYER) runs the same forward as one tile-GEMM launch per layer with small row kernels
// between the networks: the fallback for a hidden width above 256 or an observation too wide for the LDS budget, and the
// baseline the fused kernel is measured against.
//
// The constrained members (ddpg_lag.py, td3_lag.py, ddpg_pid.py, td3_pid.py) add three pieces further down: the cost
// normaliser inside td3_store_kernel (td3_cn_push), td3_multiplier_kernel -- the Adam or PID step of the multiplier on
// the windowed mean episode cost, one single-wave launch per update round -- and the actor step on reward critic 0 and
// the cost critic, whose layer-0 data gradient runs as td3_lag_dact_kernel (one K-concatenated MFMA tile over the action
// columns staged in LDS) or as two dX problems and td3_lag_dpi_kernel.
#include <math.h>

#include "offpolicy_shared.h"

namespace {

struct TLayout {
  CNet pi, q;
  int D, A, B, nq, cost, nc, ldsa, lda, ldxin;
};

int td3_make_layout(const osa_td3_desc* d, TLayout* lo) {
  if (!d) return OSA_EINVAL;
  if (d->obs_dim < 1 || d->obs_dim > 4096 || d->act_dim < 1 || d->batch < 1) return OSA_EINVAL;
  if (d->use_cost < 0 || d->use_cost > 1) return OSA_EINVAL;
  if (d->act_dim > 32 || d->batch > (1 << 20) || d->num_critics < 1 || d->num_critics > 2) return OSA_EUNSUPPORTED;
  for (int k = 0; k < 2; ++k)
    if (d->n_hidden[k] < 1 || d->n_hidden[k] + 1 > GM_MAXL) return OSA_EUNSUPPORTED;
  lo->D = d->obs_dim; lo->A = d->act_dim; lo->B = d->batch; lo->nq = d->num_critics; lo->cost = d->use_cost;
  lo->nc = lo->nq + lo->cost;
  lo->ldsa = c4(lo->D + lo->A); lo->lda = c4(lo->A); lo->ldxin = lo->ldsa + 4;
  int width[GM_MAXL], rc;
  const int na = d->n_hidden[0], nq = d->n_hidden[1];
  for (int l = 0; l < na; ++l) width[l] = d->hidden[0][l];
  width[na] = lo->A;
  if ((rc = crr_make_net(lo->pi, lo->D, na + 1, width, d->activation[0], lo->A, false)) != OSA_OK) return rc;
  for (int l = 0; l < nq; ++l) width[l] = d->hidden[1][l];
  width[nq] = 1;
  return crr_make_net(lo->q, lo->D + lo->A, nq + 1, width, d->activation[1], 1, false);
}

// ---- the workspace -----------------------------------------------------------------------------------------------
struct TWs {
  size_t xq, xc, xn[2], rcd, ho[3][GM_MAXL], ht[3][GM_MAXL], ha[2][GM_MAXL], hp[GM_MAXL], hq[GM_MAXL];
  size_t z[3][2], dx, gq, gp, rows, part, hstride, zstride, total;
};
TWs td3_ws(const TLayout& lo) {
  TWs w = {};
  size_t off = 0;
  auto take = [&](size_t n) {
    const size_t o = off;
    off += (n + 3) / 4 * 4;
    return o;
  };
  const size_t B = lo.B;
  w.xq = take(B * lo.ldsa); w.xc = take(B * lo.ldsa);
  for (int g = 0; g < 2; ++g) w.xn[g] = take(B * lo.ldsa);
  w.rcd = take(3 * B);
  for (int j = 0; j < 3; ++j)  // (the fused kernel addresses net j's outputs as ho[0] + j hstride)
    for (int l = 0; l < GM_MAXL; ++l) w.ho[j][l] = l < lo.q.L ? take(B * lo.q.ldh[l]) : 0;
  w.hstride = w.ho[1][0] - w.ho[0][0];
  for (int j = 0; j < 3; ++j)
    for (int l = 0; l < GM_MAXL; ++l) w.ht[j][l] = l < lo.q.L ? take(B * lo.q.ldh[l]) : 0;
  for (int g = 0; g < 2; ++g)
    for (int l = 0; l < GM_MAXL; ++l) w.ha[g][l] = l < lo.pi.L ? take(B * lo.pi.ldh[l]) : 0;
  for (int l = 0; l < GM_MAXL; ++l) w.hp[l] = l < lo.pi.L ? take(B * lo.pi.ldh[l]) : 0;
  for (int l = 0; l < GM_MAXL; ++l) w.hq[l] = l < lo.q.L ? take(B * lo.q.ldh[l]) : 0;
  const int mz = lo.pi.maxldh > lo.q.maxldh ? lo.pi.maxldh : lo.q.maxldh;
  for (int j = 0; j < 3; ++j)
    for (int k = 0; k < 2; ++k) w.z[j][k] = take(B * mz);
  w.zstride = w.z[1][0] - w.z[0][0];
  w.dx = take(B * lo.ldsa);
  w.gq = take((size_t)3 * lo.q.P);
  w.gp = take(lo.pi.P);
  w.rows = take(3 * B);
  w.part = take((size_t)3 * T_NB * 2 * 2);  // [group][T_NB][2] doubles
  w.total = off;
  return w;
}

// ---- the step's scalar algebra, shared by both routes ----------------------------------------------------------------
// td3.py:80-84: (a + clamp(policy_noise eps, -clip, clip)) clamped to [-1, 1]
__device__ __forceinline__ float td3_noisy(float a, float eps, float pn, float clip) {
  const float nz = fminf(fmaxf(__fmul_rn(eps, pn), -clip), clip);
  return fminf(fmaxf(__fadd_rn(a, nz), -1.f), 1.f);
}

// ---- the fused forward ---------------------------------------------------------------------------------------------
size_t td3_fwd_lds(const TLayout& lo) {
  return sizeof(float) * ((size_t)2 * BC_ROWS * BC_LDH + BC_PART + 5 * BC_ROWS + (size_t)BC_ROWS * lo.ldxin);
}
bool td3_chain_ok(const TLayout& lo) {
  for (const CNet* n : {&lo.pi, &lo.q})
    for (int l = 0; l + 1 < n->L; ++l)
      if (n->out[l] > BC_MAXW) return false;
  return td3_fwd_lds(lo) <= (size_t)BC_LDS_DYN;
}

struct TFwd {
  osa_td3_ring r;
  const long* idx;
  const float* eps;
  const long* step;
  BNetK net[2];         // actor, critic
  const float* pa[2];   // the actor of the reward target, of the cost target
  const float* pt[3];   // target critics: reward ..., cost
  const float* po[3];   // online critics, same order
  float *xq, *ho0, *dz0, *rows;
  long hstride, zstride;
  int hoff[GM_MAXL], ldh[GM_MAXL];  // layer l of online critic j: ho0 + j hstride + hoff[l], rows of ldh[l] floats
  int nslots, nq, cost, share, noise, D, A, B, ldxin, ldsa;
  float pn, pclip, gamma, inv2B;
};

// hidden layer of an online critic: into the other ping-pong buffer AND once to the workspace (the backward reads it)
struct TEmitStore {
  float *dst, *out;
  int N, act, ldo, m0, B;
  __device__ __forceinline__ void operator()(int row, int n, float v) const {
    if (n >= ((N + 3) & ~3)) return;
    const float h = n < N ? gm_act(v, act) : 0.f;
    dst[row * BC_LDH + n] = h;
    if (m0 + row < B) out[(long)(m0 + row) * ldo + n] = h;
  }
};

__global__ __launch_bounds__(256) void td3_forward_kernel(TFwd g) {
  extern __shared__ __attribute__((aligned(16))) float t_smem[];
  __shared__ BNetK nets[2];  // (a run-time layer index into the by-value argument would go through scratch memory)
  __shared__ int hoff[GM_MAXL], ldh[GM_MAXL];
  __shared__ long gi[BC_ROWS];
  float* hb0 = t_smem;
  float* hb1 = hb0 + BC_ROWS * BC_LDH;
  float* part = hb1 + BC_ROWS * BC_LDH;
  float* qv = part + BC_PART;      // [3][32] the target critics' values
  float* yv = qv + 3 * BC_ROWS;    // [2][32] the TD targets
  float* xin = yv + 2 * BC_ROWS;   // [32][ldxin] next_obs || a', then obs || act
  const int tid = threadIdx.x, m0 = blockIdx.x * BC_ROWS;
  const int D = g.D, A = g.A, B = g.B, ldxin = g.ldxin, nq = g.nq;
  if (tid == 0) {
    nets[0] = g.net[0];
    nets[1] = g.net[1];
  }
  if (tid < GM_MAXL) {
    hoff[tid] = g.hoff[tid];
    ldh[tid] = g.ldh[tid];
  }
  const long slot = *g.step % g.nslots;
  if (tid < BC_ROWS) {
    long i = 0;
    if (m0 + tid < B) {
      i = g.idx[slot * B + m0 + tid];
      if (i < 0 || i >= g.r.size) i = 0;  // (injected indices are checked on the host; never read outside the ring)
    }
    gi[tid] = i;
  }
  __syncthreads();
  const float* __restrict__ eps = g.eps + slot * (long)B * A;
  for (int e = tid; e < BC_ROWS * ldxin; e += 256) {
    const int r = e / ldxin, c = e - r * ldxin;
    xin[e] = (m0 + r < B && c < D) ? g.r.next_obs[gi[r] * g.r.ld_obs + c] : 0.f;
  }
  __syncthreads();
  // ---- the target chain on next_obs
  const int lda4 = (D + A + 3) & ~3;
  const float pn = g.pn, pclip = g.pclip;
  for (int grp = 0; grp <= g.cost; ++grp) {
    if (grp == 0 || !g.share) {
      const bool noise = grp == 0 && g.noise;
      bc_net(&nets[0], grp == 0 ? g.pa[0] : g.pa[1], xin, ldxin, hb0, hb1, part, [=](int row, int n, float v) {
        if (n < A) {
          float a = gm_act(v, OSA_ACT_TANH);
          if (noise && m0 + row < B) a = td3_noisy(a, eps[(long)(m0 + row) * A + n], pn, pclip);
          xin[row * ldxin + D + n] = a;
        } else if (D + n < lda4) {
          xin[row * ldxin + D + n] = 0.f;
        }
      });
    }
    const int k0 = grp == 0 ? 0 : nq, k1 = grp == 0 ? nq : nq + 1;
    for (int k = k0; k < k1; ++k) {
      float* qk = qv + k * BC_ROWS;
      bc_net(&nets[1], k == 0 ? g.pt[0] : (k == 1 ? g.pt[1] : g.pt[2]), xin, ldxin, hb0, hb1, part,
             [=](int row, int n, float v) {
               if (n == 0) qk[row] = v;
             });
    }
  }
  if (tid < BC_ROWS && m0 + tid < B) {
    const long i = gi[tid];
    const float done = g.r.done[i];
    const float qm = nq == 2 ? fminf(qv[tid], qv[BC_ROWS + tid]) : qv[tid];
    yv[tid] = td3_y(g.r.reward[i], done, g.gamma, qm);
    if (g.cost) yv[BC_ROWS + tid] = td3_y(g.r.cost[i], done, g.gamma, qv[nq * BC_ROWS + tid]);
  }
  // ---- the online critics on obs || act of the same rows (the last layer's barrier: every read of xin is done)
  for (int e = tid; e < BC_ROWS * ldxin; e += 256) {
    const int r = e / ldxin, c = e - r * ldxin, m = m0 + r;
    float v = 0.f;
    if (m < B) {
      if (c < D) v = g.r.obs[gi[r] * g.r.ld_obs + c];
      else if (c < D + A) v = g.r.act[gi[r] * g.r.ld_act + c - D];
      if (c < g.ldsa) g.xq[(long)m * g.ldsa + c] = v;
    }
    xin[e] = v;
  }
  __syncthreads();
  const int L = __builtin_amdgcn_readfirstlane(nets[1].L), act = __builtin_amdgcn_readfirstlane(nets[1].act);
  const float inv2B = g.inv2B;
  for (int j = 0; j < nq + g.cost; ++j) {
    const float* __restrict__ p = j == 0 ? g.po[0] : (j == 1 ? g.po[1] : g.po[2]);
    float* hj = g.ho0 + j * g.hstride;
    float* dz = g.dz0 + j * g.zstride;
    float* rows = g.rows + (long)j * B;
    const float* y = yv + (j < nq ? 0 : BC_ROWS);
    for (int l = 0; l < L; ++l) {
      const int N = __builtin_amdgcn_readfirstlane(nets[1].N[l]), ld = __builtin_amdgcn_readfirstlane(nets[1].ld[l]);
      const float* W = p + __builtin_amdgcn_readfirstlane(nets[1].oW[l]);
      const float* b = p + __builtin_amdgcn_readfirstlane(nets[1].ob[l]);
      const float* src = l == 0 ? xin : ((l & 1) ? hb0 : hb1);
      const int lds = l == 0 ? ldxin : BC_LDH;
      float* out = hj + __builtin_amdgcn_readfirstlane(hoff[l]);
      if (l + 1 < L) {
        bc_layer(W, b, N, ld, src, lds, part,
                 TEmitStore{(l & 1) ? hb1 : hb0, out, N, act, __builtin_amdgcn_readfirstlane(ldh[l]), m0, B});
      } else {
        bc_layer(W, b, N, ld, src, lds, part, [=](int row, int n, float v) {
          const int m = m0 + row;
          if (n != 0 || m >= B) return;
          const float e = v - y[row];
          const f32x4 qo = {v, 0.f, 0.f, 0.f}, d = {e * inv2B, 0.f, 0.f, 0.f};
          *reinterpret_cast<f32x4*>(out + 4 * (long)m) = qo;
          *reinterpret_cast<f32x4*>(dz + 4 * (long)m) = d;
          rows[m] = e * e;
        });
      }
    }
  }
}

// ---- the layer route's row kernels (the gather: offpolicy_shared.h) ----------------------------------------------------
// x[b][D + j] = the target action of the head's pre-activation pre[b][j]; eps != null: with the clipped noise
__global__ __launch_bounds__(256) void td3_action_kernel(int B, int A, int D, int lda, int ldsa,
                                                         const float* __restrict__ pre, const float* __restrict__ eps,
                                                         const long* __restrict__ step, int nslots, float pn, float pclip,
                                                         float* __restrict__ x) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= B * A) return;
  const int b = e / A, j = e - b * A;
  float a = gm_act(pre[(long)b * lda + j], OSA_ACT_TANH);
  if (eps) a = td3_noisy(a, eps[(*step % nslots) * (long)B * A + e], pn, pclip);
  x[(long)b * ldsa + D + j] = a;
}
struct TTd {
  const float* q[3];   // [B][4] online critics
  const float* tq[3];  // [B][4] target critics
  const float* rcd;
  float* dz[3];
  float* rows;
  int B, nq, cost;
  float gamma;
};
__global__ __launch_bounds__(256) void td3_td_kernel(TTd g) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= g.B) return;
  const float done = g.rcd[2 * g.B + b], inv2B = 2.f / (float)g.B;
  const float qm = g.nq == 2 ? fminf(g.tq[0][4 * b], g.tq[1][4 * b]) : g.tq[0][4 * b];
  const float yr = td3_y(g.rcd[b], done, g.gamma, qm);
  const float yc = g.cost ? td3_y(g.rcd[g.B + b], done, g.gamma, (g.nq == 2 ? g.tq[2] : g.tq[1])[4 * b]) : 0.f;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    if (j >= g.nq + g.cost) break;
    const float e = g.q[j][4 * b] - (j < g.nq ? yr : yc);
    const f32x4 d = {e * inv2B, 0.f, 0.f, 0.f};
    *reinterpret_cast<f32x4*>(g.dz[j] + 4 * b) = d;
    g.rows[(long)j * g.B + b] = e * e;
  }
}

// ---- the actor step's row kernels --------------------------------------------------------------------------------
// xc = obs || tanh(pre) (pre overwritten with the tanh: the backward reads it); dz = d(-mean q)/dq
__global__ __launch_bounds__(256) void td3_pi_kernel(int B, int A, int D, int lda, int ldsa, float* __restrict__ pre,
                                                     const float* __restrict__ xq, float* __restrict__ xc,
                                                     float* __restrict__ dz) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= B * ldsa) return;
  const int b = e / ldsa, c = e - b * ldsa;
  float v = 0.f;
  if (c < D) {
    v = xq[e];
  } else if (c < D + A) {
    v = gm_act(pre[(long)b * lda + c - D], OSA_ACT_TANH);
    pre[(long)b * lda + c - D] = v;
  }
  xc[e] = v;
  if (c == 0) {
    const f32x4 d = {-1.f / (float)B, 0.f, 0.f, 0.f};
    *reinterpret_cast<f32x4*>(dz + 4 * (long)b) = d;
  }
}
// dL/d(head pre-activation) = dL/da (1 - tanh^2); padding zero
__global__ __launch_bounds__(256) void td3_dpi_kernel(int B, int A, int D, int lda, int ldsa,
                                                      const float* __restrict__ dx, const float* __restrict__ th,
                                                      float* __restrict__ dz) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= B * lda) return;
  const int b = e / lda, j = e - b * lda;
  float d = 0.f;
  if (j < A) {
    const float t = th[e];
    d = dx[(long)b * ldsa + D + j] * (1.f - t * t);
  }
  dz[e] = d;
}
// (td3_critic_dx, the norm, Adam and finish kernels: offpolicy_shared.h)

// ---- the constrained actor step (ddpg_lag.py:73-100) -----------------------------------------------------------------
// Extra workspace behind TD3's: the cost critic's layer outputs on obs || pi(obs), its input gradient (the stacked
// composition only) and the rows' negated loss terms [B][4], which the actor's Adam launch averages.
struct TLagWs {
  size_t hqc[GM_MAXL], dxc, nl, dzpi, total;
};
TLagWs td3_lag_ws(const TLayout& lo, const TWs& w) {
  TLagWs x = {};
  size_t off = w.total;
  auto take = [&](size_t n) {
    const size_t o = off;
    off += (n + 3) / 4 * 4;
    return o;
  };
  const size_t B = lo.B;
  for (int l = 0; l < GM_MAXL; ++l) x.hqc[l] = l < lo.q.L ? take(B * lo.q.ldh[l]) : 0;
  x.dxc = take(B * lo.ldsa);
  x.nl = take(4 * B);
  x.dzpi = take(B * lo.pi.maxldh);  // the head's dz: with one hidden actor layer no backward writes it again
  x.total = off;
  return x;
}

// loss row b = (-q_r + lambda q_c) / (1 + lambda); its negative goes to nl[b][0] (the Adam launch logs -mean), the two
// top-layer gradients d loss / d q to dzr and dzc
__global__ __launch_bounds__(256) void td3_lag_row_kernel(int B, const float* __restrict__ lambda,
                                                          const float* __restrict__ qr, const float* __restrict__ qc,
                                                          float* __restrict__ dzr, float* __restrict__ dzc,
                                                          float* __restrict__ nl) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const float lam = *lambda, inv = 1.f / (1.f + lam), invB = inv / (float)B;
  const f32x4 dr = {-invB, 0.f, 0.f, 0.f}, dc = {lam * invB, 0.f, 0.f, 0.f};
  const f32x4 l = {(qr[4 * (long)b] - lam * qc[4 * (long)b]) * inv, 0.f, 0.f, 0.f};
  *reinterpret_cast<f32x4*>(dzr + 4 * (long)b) = dr;
  *reinterpret_cast<f32x4*>(dzc + 4 * (long)b) = dc;
  *reinterpret_cast<f32x4*>(nl + 4 * (long)b) = l;
}

// Layer 0 of both critics' data gradient, straight to the actor head's dz:
//   dz[b][j] = (sum_n dZ0_r[b][n] W0_r[n][D + j] + sum_n dZ0_c[b][n] W0_c[n][D + j]) (1 - th[b][j]^2),  j < A <= 32
// ONE GEMM with K concatenated over both critics and a single 32-column MFMA tile of output: the D observation columns
// that two full-width dX GEMMs would compute and nobody reads are never formed, and the sum and the tanh' ride on the
// write-back.  A workgroup of four waves owns 32 rows.  The B operand -- the action columns W0[:, D : D + A], a walk of
// stride ld in global memory -- is staged once per workgroup into LDS as [k][32] (row stride 40 floats: the two lane
// groups of an MFMA step read rows 4 apart = 160 floats, 32 banks apart), DA_KC rows at a time, a wider slab in chunks;
// the A operand, rows of dZ0, comes from global memory as 16-byte loads along K into float32 32x32x2 MFMAs.  K of a chunk
// is split over the four waves; the partial tiles meet in LDS and are added in wave order (chain_layer.h's one-tile
// branch).  No atomics, no cooperative groups, no spin-waits.
// LDS: DA_KC x 40 floats of slab (40 KB) + 4 partial tiles (16 KB) = 56 KB static.
constexpr int DA_KC = 256, DA_LD = 40;
struct TDact {
  const float* dz0[2];  // [B][ldz]: dL/d(layer 0's pre-activation) of the reward critic, of the cost critic
  const float* W0[2];   // [H][ldw]: their first layers
  const float* th;      // [B][lda] tanh of the actor's head
  float* dz;            // [B][lda]
  int B, A, D, H, ldz, ldw, lda;
};
__global__ __launch_bounds__(256) void td3_lag_dact_kernel(TDact g) {
  __shared__ __attribute__((aligned(16))) float slab[DA_KC * DA_LD];
  __shared__ float part[BC_PART];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, kk = lane >> 5;
  const int m0 = blockIdx.x * BC_ROWS, H = g.H;
  const bool rok = m0 + l31 < g.B;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int c = 0; c < 2; ++c) {
    const float* __restrict__ W = c == 0 ? g.W0[0] : g.W0[1];
    const float* __restrict__ arow = (c == 0 ? g.dz0[0] : g.dz0[1]) + (long)(m0 + l31) * g.ldz + 4 * kk;
    for (int k0 = 0; k0 < H; k0 += DA_KC) {
      const int live = H - k0 < DA_KC ? H - k0 : DA_KC, nks = (live + 7) >> 3;  // K steps of 8 in this chunk
      // stage rows k0 .. k0 + 8 nks of the action columns; rows past H and columns past A are zero
      for (int k = tid >> 5; k < 8 * nks; k += 8)
        slab[k * DA_LD + l31] = (k < live && l31 < g.A) ? W[(long)(k0 + k) * g.ldw + g.D + l31] : 0.f;
      __syncthreads();
      const int per = (nks + 3) >> 2, s0 = wave * per, s1 = s0 + per < nks ? s0 + per : nks;
      for (int s = s0; s < s1; ++s) {
        const int k = 8 * s + 4 * kk;  // this lane group's four K values of the step (within the chunk)
        f32x4 af = (rok && k0 + k < g.ldz) ? *reinterpret_cast<const f32x4*>(arow + k0 + 8 * s) : zero;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (k + q >= live) af[q] = 0.f;  // (a dX launch leaves the padding columns of dZ0 unwritten)
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[q], slab[(k + q) * DA_LD + l31], acc, 0, 0, 0);
        }
      }
      __syncthreads();  // the slab is free for the next chunk
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) part[(wave * 16 + r) * 64 + lane] = acc[r];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = 4 * wave + i, m = m0 + (r & 3) + 8 * (r >> 2) + 4 * kk;
    float v = part[(0 * 16 + r) * 64 + lane];
    v += part[(1 * 16 + r) * 64 + lane];
    v += part[(2 * 16 + r) * 64 + lane];
    v += part[(3 * 16 + r) * 64 + lane];
    if (m < g.B && l31 < g.lda) {
      float d = 0.f;
      if (l31 < g.A) {
        const float t = g.th[(long)m * g.lda + l31];
        d = v * (1.f - t * t);
      }
      g.dz[(long)m * g.lda + l31] = d;
    }
  }
}
// the stacked composition's row kernel: dz = (dx_r + dx_c)[action columns] (1 - tanh^2); padding zero
__global__ __launch_bounds__(256) void td3_lag_dpi_kernel(int B, int A, int D, int lda, int ldsa,
                                                          const float* __restrict__ dxr, const float* __restrict__ dxc,
                                                          const float* __restrict__ th, float* __restrict__ dz) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= B * lda) return;
  const int b = e / lda, j = e - b * lda;
  float d = 0.f;
  if (j < A) {
    const float t = th[e];
    d = (dxr[(long)b * ldsa + D + j] + dxc[(long)b * ldsa + D + j]) * (1.f - t * t);
  }
  dz[e] = d;
}

// ---- the multiplier (common/lagrange.py:95-136, common/pid_lagrange.py:98-146) ---------------------------------------
struct TMult {
  osa_td3_lag L;
  const float *carry, *ep_out;
  const long *ep_count, *step;
  float* stats;
  long ep_cap;
  int ncarry, update, nslots;
};
__global__ __launch_bounds__(64) void td3_multiplier_kernel(TMult g) {
  if (threadIdx.x != 0) return;
  const osa_td3_lag& L = g.L;
  long ne = *g.ep_count;
  if (ne > g.ep_cap) ne = g.ep_cap;
  if (ne < 0) ne = 0;
  const long total = g.ncarry + ne, first = total > L.window_lens ? total - L.window_lens : 0;
  if (g.update && total > 0) {
    double sum = 0.0;  // oldest first
    for (long i = first; i < total; ++i)
      sum = __dadd_rn(sum, (double)(i < g.ncarry ? g.carry[i] : g.ep_out[3 * (i - g.ncarry) + 1]));
    const double Jc = __ddiv_rn(sum, (double)(total - first));
    const int t = *L.count;
    if (L.mode == OSA_TD3_LAG_ADAM) {  // the gradient of -lambda (Jc - limit), rounded to float32 as autograd leaves it
      const float grad = (float)(-(__dsub_rn(Jc, L.cost_limit)));
      const float b2 = (float)0.999, omb1 = (float)(1.0 - 0.9), omb2 = (float)(1.0 - 0.999);
      float m = L.adam[0], v = L.adam[1];
      m = __fadd_rn(m, __fmul_rn(__fsub_rn(grad, m), omb1));                      // exp_avg.lerp_(grad, 1 - beta1)
      v = __fadd_rn(__fmul_rn(v, b2), __fmul_rn(__fmul_rn(omb2, grad), grad));  // .mul_(beta2).addcmul_(g, g, 1 - beta2)
      const double bc1 = 1.0 - pow(0.9, (double)(t + 1)), bc2 = 1.0 - pow(0.999, (double)(t + 1));
      const float step_size = (float)(L.lambda_lr / bc1), bc2_sqrt = (float)sqrt(bc2);
      const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(v), bc2_sqrt), (float)1e-8);
      float lam = __fsub_rn(*L.multiplier, __fmul_rn(step_size, __fdiv_rn(m, denom)));
      lam = fmaxf(lam, 0.f);
      if (L.upper_bound >= 0.0) lam = fminf(lam, (float)L.upper_bound);
      L.adam[0] = m; L.adam[1] = v;
      *L.multiplier = lam;
    } else {  // pid_lagrange.py::pid_step, in double and in its order
      double* s = L.pid;
      double* hist = s + 3;
      const int depth = L.pid_d_delay;
      const double err = __dsub_rn(Jc, L.cost_limit);
      double integral = fmax(0.0, __dadd_rn(s[0], __dmul_rn(err, L.ki)));
      if (L.diff_norm) integral = fmax(0.0, fmin(1.0, integral));
      const double err_ema = __dadd_rn(__dmul_rn(s[1], L.alpha_p), __dmul_rn(__dsub_rn(1.0, L.alpha_p), err));
      const double cost_ema = __dadd_rn(__dmul_rn(s[2], L.alpha_d), __dmul_rn(__dsub_rn(1.0, L.alpha_d), Jc));
      const int oldest = t + 1 - depth > 0 ? t + 1 - depth : 0;  // history = the last `depth` of {0, ema_1, .., ema_t}
      const double rise = fmax(0.0, __dsub_rn(cost_ema, hist[oldest % depth]));
      double out = fmax(0.0, __dadd_rn(__dadd_rn(__dmul_rn(L.kp, err_ema), integral), __dmul_rn(L.kd, rise)));
      if (L.diff_norm) out = fmin(1.0, out);
      else if (!L.sum_norm) out = fmin(out, L.penalty_max);
      hist[(t + 1) % depth] = cost_ema;
      s[0] = integral; s[1] = err_ema; s[2] = cost_ema;
      *L.multiplier = (float)out;
    }
    *L.count = t + 1;
  }
  const long done = *g.step > 0 ? *g.step - 1 : 0;
  g.stats[(done % g.nslots) * OSA_TD3_NSTAT + OSA_TD3_LAG_COL] = *L.multiplier;
}

// ---- ring, draws, act ------------------------------------------------------------------------------------------------
struct TStore {
  osa_td3_ring r;
  int n, D, A, ld_obs, ld_act, ld_next, ld_final;
  const float *obs, *act, *reward, *cost, *next_obs, *final_obs;
  const unsigned char *term, *trunc, *final_mask;
  float *ep_acc, *ep_out;
  long ep_cap;
  long* ep_count;
  double* cn;  // the cost normaliser {mean, sumsq, count}, or null
};
// Normalizer._push of the n raw costs (normalizer.py:110-139) by one thread, in double with every operation rounded on
// its own (no contraction: a float64 restatement on the host gives the same bits); out = {mean, std, count}
__device__ void td3_cn_push(double* cn, const float* __restrict__ cost, int n, double* out) {
  double sum = 0.0;
  for (int i = 0; i < n; ++i) sum = __dadd_rn(sum, (double)cost[i]);
  const double mean_raw = __ddiv_rn(sum, (double)n);
  double sq = 0.0;
  for (int i = 0; i < n; ++i) {
    const double d = __dsub_rn((double)cost[i], mean_raw);
    sq = __dadd_rn(sq, __dmul_rn(d, d));
  }
  double mean = mean_raw, sumsq = sq, count = (double)n;
  if (cn[2] > 0.0) {  // the pairwise update of Chan, Golub and LeVeque
    const double old = cn[2], delta = __dsub_rn(mean_raw, cn[0]);
    count = __dadd_rn(old, (double)n);
    mean = __dadd_rn(cn[0], __ddiv_rn(__dmul_rn(delta, (double)n), count));
    const double cross = __ddiv_rn(__dmul_rn(__dmul_rn(__dmul_rn(delta, delta), old), (double)n), count);
    sumsq = __dadd_rn(cn[1], __dadd_rn(sq, cross));
  }
  cn[0] = mean; cn[1] = sumsq; cn[2] = count;
  out[0] = mean;
  out[1] = count > 1.0 ? fmax(__dsqrt_rn(__ddiv_rn(sumsq, __dsub_rn(count, 1.0))), 1e-2) : 1.0;
  out[2] = count;
}
__global__ __launch_bounds__(256) void td3_store_kernel(TStore g) {
  __shared__ double cn[3];
  const long pos = g.r.pos[0], fill = g.r.pos[1];
  if (g.cn) {
    if (threadIdx.x == 0) td3_cn_push(g.cn, g.cost, g.n, cn);
    __syncthreads();
  }
  const int W = g.D + g.A + g.D;
  for (int e = threadIdx.x; e < g.n * W; e += 256) {
    const int i = e / W, c = e - i * W;
    const long row = (pos + i) % g.r.size;
    if (c < g.D) {
      g.r.obs[row * g.r.ld_obs + c] = g.obs[(long)i * g.ld_obs + c];
    } else if (c < g.D + g.A) {
      g.r.act[row * g.r.ld_act + c - g.D] = g.act[(long)i * g.ld_act + c - g.D];
    } else {
      const int k = c - g.D - g.A;
      // (the value is selected, not the address: a per-lane choice between the two uniform base pointers came out of
      // the compiler as one scalar base for the whole wave)
      float v = g.next_obs[(long)i * g.ld_next + k];
      if (g.final_obs && g.final_mask[i]) v = g.final_obs[(long)i * g.ld_final + k];
      g.r.next_obs[row * g.r.ld_obs + k] = v;
    }
  }
  for (int i = threadIdx.x; i < g.n; i += 256) {
    const long row = (pos + i) % g.r.size;
    g.r.reward[row] = g.reward[i];
    float c = g.cost[i];
    if (g.cn && cn[2] > 1.0)  // Normalizer.normalize, clip 5; count <= 1: the raw cost
      c = (float)fmin(fmax(__ddiv_rn(__dsub_rn((double)c, cn[0]), cn[1]), -5.0), 5.0);
    g.r.cost[row] = c;
    g.r.done[row] = g.term[i] ? 1.f : 0.f;
  }
  __syncthreads();  // every thread has read the position
  if (threadIdx.x == 0) {
    g.r.pos[0] = (pos + g.n) % g.r.size;
    g.r.pos[1] = fill + g.n < g.r.size ? fill + g.n : g.r.size;
    if (g.ep_acc) {  // the envs in order: the episodes' order in ep_out is fixed
      long cnt = *g.ep_count;
      for (int i = 0; i < g.n; ++i) {
        float* a = g.ep_acc + 3 * i;
        a[0] += g.reward[i];
        a[1] += g.cost[i];
        a[2] += 1.f;
        if (g.term[i] || g.trunc[i]) {
          if (cnt < g.ep_cap)
            for (int k = 0; k < 3; ++k) g.ep_out[3 * cnt + k] = a[k];
          ++cnt;
          a[0] = a[1] = a[2] = 0.f;
        }
      }
      *g.ep_count = cnt;
    }
  }
}

#define TD3_KEY_IDX 0x54443349445831ull /* keys of their own: seed ^ key, counter = (step, element) */
#define TD3_KEY_EPS 0x54443345505331ull
#define TD3_KEY_ACT 0x54443341435431ull

__global__ __launch_bounds__(256) void td3_draw_kernel(unsigned long long seed, long first, int nsteps, int nslots, int B,
                                                       int A, const long* __restrict__ pos, long* __restrict__ idx,
                                                       float* __restrict__ eps) {
  const long per = (long)B * (1 + A), e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= nsteps * per) return;
  const long k = e / per, i = e - k * per, step = first + k, slot = step % nslots;
  uint32_t w[4];
  if (i < B) {
    const long fill = pos[1] > 0 ? pos[1] : 1;
    osa_philox(seed ^ TD3_KEY_IDX, (uint64_t)step, (uint64_t)i, w);
    const unsigned long long bits = (unsigned long long)w[0] | ((unsigned long long)w[1] << 32);
    idx[slot * B + i] = (long)__umul64hi(bits, (unsigned long long)fill);
  } else {
    osa_philox(seed ^ TD3_KEY_EPS, (uint64_t)step, (uint64_t)(i - B), w);
    eps[slot * (long)B * A + (i - B)] = td3_normal(w);
  }
}

// one row per workgroup; a wave per output column, lanes over K, the wave's sum in a fixed order
struct TAct {
  BNetK net;
  const float *p, *obs;
  float* out;
  int D, A, ld_obs, ld_out, mode;
  float noise;
  unsigned long long key, offset;
};
constexpr int T_ACT_W = 4096;
__global__ __launch_bounds__(256) void td3_act_kernel(TAct g) {
  __shared__ float buf[2][T_ACT_W];
  __shared__ BNetK nk;
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t w[4];
  if (g.mode == 1) {  // use_rand_action: uniform over the action box [-1, 1]
    if (tid < g.A) {
      osa_philox(g.key, g.offset, (uint64_t)row * g.A + tid, w);
      g.out[(long)row * g.ld_out + tid] = __fsub_rn(__fmul_rn(2.f, osa_u01(w[0])), 1.f);
    }
    return;
  }
  if (tid == 0) nk = g.net;
  for (int c = tid; c < g.D; c += 256) buf[0][c] = g.obs[(long)row * g.ld_obs + c];
  __syncthreads();
  int cur = 0, K = g.D;
  for (int l = 0; l < nk.L; ++l) {
    const int N = nk.N[l], ld = nk.ld[l];
    const float* __restrict__ W = g.p + nk.oW[l];
    const float* __restrict__ b = g.p + nk.ob[l];
    for (int n = wave; n < N; n += 4) {
      float s = 0.f;
      for (int k = lane; k < K; k += 64) s = fmaf(W[(long)n * ld + k], buf[cur][k], s);
      s = osa_wave_sum(s);
      if (lane == 0) buf[cur ^ 1][n] = gm_act(s + b[n], l + 1 < nk.L ? nk.act : OSA_ACT_TANH);
    }
    __syncthreads();
    cur ^= 1;
    K = N;
  }
  if (tid < g.A) {
    float a = buf[cur][tid];
    if (g.noise > 0.f) {  // MLPActor.predict(deterministic=False): clamp(a + N(0, noise), -1, 1)
      osa_philox(g.key, g.offset, (uint64_t)row * g.A + tid, w);
      a = fminf(fmaxf(__fadd_rn(a, __fmul_rn(g.noise, td3_normal(w))), -1.f), 1.f);
    }
    g.out[(long)row * g.ld_out + tid] = a;
  }
}

int td3_route_ok(const TLayout& lo, int route) {
  if (route != OSA_TD3_ROUTE_LAYER && route != OSA_TD3_ROUTE_FUSED) return OSA_EINVAL;
  return route == OSA_TD3_ROUTE_FUSED && !td3_chain_ok(lo) ? OSA_EUNSUPPORTED : OSA_OK;
}

// the forward of a step on either route: leaves xq, the online critics' layer outputs ho, dq in z[j][0] and the rows'
// squared errors
int td3_forward(const TLayout& lo, const TWs& w, const osa_td3_hparams* hp, const osa_td3_state* s,
                const osa_td3_ring* ring, const osa_td3_draw_buffers* dr, float* ws, hipStream_t st) {
  const int B = lo.B, top = lo.q.L - 1, nq = lo.nq, nc = lo.nc;
  const long Pc = lo.q.P;
  const bool noise = hp->policy_noise > 0.f;
  const float* pa0 = hp->target_actor ? s->actor_t : s->actor;
  const bool share = lo.cost && !hp->target_actor && !noise;  // (DDPG: both targets take the online actor's action)
  if (hp->route == OSA_TD3_ROUTE_FUSED) {
    static OsaPerDeviceOnce attr_set;
    if (attr_set.need()) {
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(&td3_forward_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, BC_LDS_DYN) != hipSuccess)
        return OSA_EHIP;
      attr_set.set();
    }
    TFwd g = {};
    g.r = *ring; g.idx = dr->idx; g.eps = dr->eps; g.step = s->step;
    g.net[0] = bcq_netk(lo.pi); g.net[1] = bcq_netk(lo.q);
    g.pa[0] = pa0; g.pa[1] = s->actor;
    for (int j = 0; j < nc; ++j) {
      g.pt[j] = s->critic_t + j * Pc;
      g.po[j] = s->critic + j * Pc;
    }
    g.xq = ws + w.xq; g.ho0 = ws + w.ho[0][0]; g.dz0 = ws + w.z[0][0]; g.rows = ws + w.rows;
    g.hstride = (long)w.hstride; g.zstride = (long)w.zstride;
    for (int l = 0; l < lo.q.L; ++l) {
      g.hoff[l] = (int)(w.ho[0][l] - w.ho[0][0]);
      g.ldh[l] = lo.q.ldh[l];
    }
    g.nslots = dr->nslots; g.nq = nq; g.cost = lo.cost; g.share = share; g.noise = noise;
    g.D = lo.D; g.A = lo.A; g.B = B; g.ldxin = lo.ldxin; g.ldsa = lo.ldsa;
    g.pn = hp->policy_noise; g.pclip = hp->policy_noise_clip; g.gamma = hp->gamma; g.inv2B = 2.f / (float)B;
    hipLaunchKernelGGL(td3_forward_kernel, dim3((B + BC_ROWS - 1) / BC_ROWS), dim3(256), td3_fwd_lds(lo), st, g);
    return hipGetLastError() == hipSuccess ? OSA_OK : OSA_EHIP;
  }
  int rc;
  const bool two = lo.cost && !share;
  TGather ga = {*ring, dr->idx, s->step, dr->nslots, B, lo.D, lo.A, lo.ldsa, ws + w.xq, ws + w.xn[0],
                two ? ws + w.xn[1] : nullptr, ws + w.rcd};
  hipLaunchKernelGGL(td3_gather_kernel, dim3(crr_blocks(B, 4)), dim3(256), 0, st, ga);
  for (int grp = 0; grp < (two ? 2 : 1); ++grp) {
    const CFwd af = {grp == 0 ? pa0 : s->actor, ws + w.xn[grp], lo.ldsa, B, w.ha[grp]};
    if ((rc = crr_forward(lo.pi, &af, 1, ws, st)) != OSA_OK) return rc;
    hipLaunchKernelGGL(td3_action_kernel, dim3(crr_blocks((long)B * lo.A, 256)), dim3(256), 0, st, B, lo.A, lo.D, lo.lda,
                       lo.ldsa, ws + w.ha[grp][lo.pi.L - 1], grp == 0 && noise ? dr->eps : (const float*)nullptr,
                       s->step, dr->nslots, hp->policy_noise, hp->policy_noise_clip, ws + w.xn[grp]);
  }
  CFwd tf[3], of[3];
  for (int j = 0; j < nc; ++j) {
    tf[j] = {s->critic_t + j * Pc, ws + w.xn[j >= nq && two ? 1 : 0], lo.ldsa, B, w.ht[j]};
    of[j] = {s->critic + j * Pc, ws + w.xq, lo.ldsa, B, w.ho[j]};
  }
  if ((rc = crr_forward(lo.q, tf, nc, ws, st)) != OSA_OK) return rc;
  if ((rc = crr_forward(lo.q, of, nc, ws, st)) != OSA_OK) return rc;
  TTd td = {};
  for (int j = 0; j < nc; ++j) {
    td.q[j] = ws + w.ho[j][top]; td.tq[j] = ws + w.ht[j][top]; td.dz[j] = ws + w.z[j][0];
  }
  td.rcd = ws + w.rcd; td.rows = ws + w.rows; td.B = B; td.nq = nq; td.cost = lo.cost; td.gamma = hp->gamma;
  hipLaunchKernelGGL(td3_td_kernel, dim3(crr_blocks(B, 256)), dim3(256), 0, st, td);
  return OSA_OK;
}

// both critics' data gradients from the top layer down to layer `stop`, two problems per launch; returns the index of
// the ping-pong buffers z[0][.] (reward critic 0) and z[2][.] (cost critic) that hold layer stop's dZ
int td3_lag_critics_dx(const TLayout& lo, const TWs& w, const TLagWs& x, const float* critic, int stop, float* ws,
                       hipStream_t st, int* cur_out) {
  const CNet& n = lo.q;
  int cur = 0;
  for (int l = n.L - 1; l >= stop; --l) {
    GArgs gd = {};
    gd.splits = 1;
    for (int k = 0; k < 2; ++k) {
      const int j = k == 0 ? 0 : 2;
      GProb q = crr_prob();  // dZ_{l-1}[rows][in] = (dZ_l[rows][out] . W_l[out][in]) * act'(H_{l-1})
      q.A = ws + w.z[j][cur]; q.lda = n.ldh[l];
      q.B = critic + (long)(k == 0 ? 0 : lo.nq) * n.P + n.oW[l]; q.ldb = n.ld[l];
      q.M = lo.B; q.N = n.in[l]; q.K = n.out[l];
      if (l > 0) {
        q.C = ws + w.z[j][cur ^ 1]; q.ldc = n.ldh[l - 1];
        q.dact = n.act; q.aux = ws + (k == 0 ? w.hq[l - 1] : x.hqc[l - 1]); q.ldaux = n.ldh[l - 1];
      } else {
        q.C = ws + (k == 0 ? w.dx : x.dxc); q.ldc = lo.ldsa;
      }
      gd.p[gd.nprob++] = q;
    }
    const int rc = gm_gemm<false, true>(gd, st);
    if (rc != OSA_OK) return rc;
    cur ^= 1;
  }
  *cur_out = cur;
  return OSA_OK;
}

int td3_lag_ok(const TLayout& lo, const osa_td3_lag* lag) {
  if (!lag->multiplier || !lo.cost) return OSA_EINVAL;
  if (lag->dact != OSA_TD3_LAG_DACT_GEMM && lag->dact != OSA_TD3_LAG_DACT_STACKED) return OSA_EINVAL;
  return lag->dact == OSA_TD3_LAG_DACT_GEMM && lo.q.out[0] > OSA_TD3_LAG_DACT_MAXW ? OSA_EUNSUPPORTED : OSA_OK;
}

}  // namespace

extern "C" {

int osa_td3_layout(const osa_td3_desc* desc, int* out) {
  TLayout lo;
  OSA_REQUIRE(desc && out);
  const int rc = td3_make_layout(desc, &lo);
  if (rc != OSA_OK) return rc;
  out[0] = lo.pi.P; out[1] = lo.q.P; out[2] = OSA_TD3_NSTAT; out[3] = 0;
  int k = 4;
  for (int net = 0; net < 2; ++net) {
    const CNet& n = net == 0 ? lo.pi : lo.q;
    for (int l = 0; l < OSA_GMLP_MAX_LAYERS; ++l) {
      out[k++] = l < n.L ? n.oW[l] : -1;
      out[k++] = l < n.L ? n.ob[l] : -1;
      out[k++] = l < n.L ? n.ld[l] : 0;
    }
  }
  return OSA_OK;
}

size_t osa_td3_ws_floats(const osa_td3_desc* desc) {
  TLayout lo;
  if (td3_make_layout(desc, &lo) != OSA_OK) return 0;
  return td3_ws(lo).total;
}

int osa_td3_chain_supported(const osa_td3_desc* desc) {
  TLayout lo;
  return td3_make_layout(desc, &lo) == OSA_OK && td3_chain_ok(lo) ? 1 : 0;
}

int osa_td3_store(const osa_td3_ring* ring, int n, int obs_dim, int act_dim, const float* obs, int ld_obs,
                  const float* act, int ld_act, const float* reward, const float* cost, const unsigned char* terminated,
                  const unsigned char* truncated, const float* next_obs, int ld_next, const float* final_obs, int ld_final,
                  const unsigned char* final_mask, float* ep_acc, float* ep_out, long ep_cap, long* ep_count, void* stream) {
  return osa_td3_store_cn(ring, n, obs_dim, act_dim, obs, ld_obs, act, ld_act, reward, cost, terminated, truncated,
                          next_obs, ld_next, final_obs, ld_final, final_mask, ep_acc, ep_out, ep_cap, ep_count, nullptr,
                          stream);
}

int osa_td3_store_cn(const osa_td3_ring* ring, int n, int obs_dim, int act_dim, const float* obs, int ld_obs,
                     const float* act, int ld_act, const float* reward, const float* cost,
                     const unsigned char* terminated, const unsigned char* truncated, const float* next_obs, int ld_next,
                     const float* final_obs, int ld_final, const unsigned char* final_mask, float* ep_acc, float* ep_out,
                     long ep_cap, long* ep_count, double* cn, void* stream) {
  OSA_REQUIRE(obs_dim >= 1 && act_dim >= 1 && td3_ring_ok(ring, obs_dim, act_dim));
  OSA_REQUIRE((reinterpret_cast<uintptr_t>(cn) & 7) == 0);
  OSA_REQUIRE(n >= 1 && n <= ring->size && obs && act && reward && cost && terminated && truncated && next_obs);
  OSA_REQUIRE(ld_obs >= obs_dim && ld_act >= act_dim && ld_next >= obs_dim);
  OSA_REQUIRE(!final_obs || (final_mask && ld_final >= obs_dim));
  OSA_REQUIRE(!ep_acc || (ep_out && ep_count && ep_cap >= 0));
  TStore g = {*ring, n, obs_dim, act_dim, ld_obs, ld_act, ld_next, ld_final, obs, act, reward, cost, next_obs, final_obs,
              terminated, truncated, final_mask, ep_acc, ep_out, ep_cap, ep_count, cn};
  hipLaunchKernelGGL(td3_store_kernel, dim3(1), dim3(256), 0, osa_stream(stream), g);
  OSA_CHECK_LAUNCH();
  return OSA_OK;
}

int osa_td3_draws(const osa_td3_desc* desc, unsigned long long seed, long first_step, int nsteps, int nslots,
                  const osa_td3_ring* ring, long* idx, float* eps, void* stream) {
  TLayout lo;
  OSA_REQUIRE(desc && idx && eps);
  const int rc = td3_make_layout(desc, &lo);
  if (rc != OSA_OK) return rc;
  OSA_REQUIRE(first_step >= 0 && nsteps >= 1 && nslots >= 1 && nsteps <= nslots && td3_ring_ok(ring, lo.D, lo.A));
  hipLaunchKernelGGL(td3_draw_kernel, dim3(crr_blocks((long)nsteps * lo.B * (1 + lo.A), 256)), dim3(256), 0,
                     osa_stream(stream), seed, first_step, nsteps, nslots, lo.B, lo.A, ring->pos, idx, eps);
  OSA_CHECK_LAUNCH();
  return OSA_OK;
}

// the step of osa_td3_step (lag null) and of osa_td3_lag_step
static int td3_step_run(const osa_td3_desc* desc, const osa_td3_hparams* hp, const osa_td3_state* s,
                        const osa_td3_lag* lag, const osa_td3_ring* ring, const osa_td3_draw_buffers* dr, float* stats,
                        float* ws, size_t ws_floats, long update_count, int nsteps, void* stream) {
  TLayout lo;
  OSA_REQUIRE(desc && hp && s && ring && dr && stats && ws && nsteps >= 1 && update_count >= 0);
  int rc = td3_make_layout(desc, &lo);
  if (rc != OSA_OK) return rc;
  if ((rc = td3_route_ok(lo, hp->route)) != OSA_OK) return rc;
  if (lag && (rc = td3_lag_ok(lo, lag)) != OSA_OK) return rc;
  const TWs w = td3_ws(lo);
  const TLagWs x = lag ? td3_lag_ws(lo, w) : TLagWs{};
  OSA_REQUIRE(ws_floats >= (lag ? x.total : w.total) && (reinterpret_cast<uintptr_t>(ws) & 15) == 0);
  OSA_REQUIRE(s->actor && s->actor_m && s->actor_v && s->actor_t && s->critic && s->critic_m && s->critic_v &&
              s->critic_t && s->adam_step && s->step);
  OSA_REQUIRE(td3_ring_ok(ring, lo.D, lo.A) && dr->idx && dr->eps && dr->nslots >= 1);
  OSA_REQUIRE(hp->policy_delay >= 1 && hp->policy_noise >= 0.f && hp->policy_noise_clip >= 0.f && hp->lr_actor >= 0.f &&
              hp->lr_critic >= 0.f && hp->max_grad_norm >= 0.f && hp->critic_norm_coeff >= 0.f && hp->beta1 >= 0.0 &&
              hp->beta1 < 1.0 && hp->beta2 >= 0.0 && hp->beta2 < 1.0);
  for (const float* p : {s->actor, s->actor_m, s->actor_v, s->actor_t, s->critic, s->critic_m, s->critic_v, s->critic_t})
    OSA_REQUIRE((reinterpret_cast<uintptr_t>(p) & 15) == 0);
  hipStream_t st = osa_stream(stream);
  const int B = lo.B, top = lo.q.L - 1, nq = lo.nq, nc = lo.nc;
  const long Pc = lo.q.P;
  double* part = reinterpret_cast<double*>(ws + w.part);
  for (int it = 0; it < nsteps; ++it) {
    const bool actor_step = (update_count + it + 1) % hp->policy_delay == 0;  // ddpg.py:398
    if ((rc = td3_forward(lo, w, hp, s, ring, dr, ws, st)) != OSA_OK) return rc;
    // ---- the critics: backward, norm (+ L2), Adam; on actor steps the Polyak update of ddpg.py:400 rides on the Adam
    // launch -- the targets are not read again in the step
    CBwd cb[3];
    for (int j = 0; j < nc; ++j)
      cb[j] = {s->critic + j * Pc, ws + w.xq, lo.ldsa, w.ho[j], {w.z[j][0], w.z[j][1]}, ws + w.gq + j * Pc};
    if ((rc = crr_backward(lo.q, cb, nc, B, ws, st)) != OSA_OK) return rc;
    TNorm nr = {{ws + w.gq, ws + w.gq + nq * Pc}, {s->critic, s->critic + nq * Pc}, {nq * Pc, Pc},
                {s->adam_step + 1, s->adam_step + 2}, part, hp->critic_norm_coeff};
    hipLaunchKernelGGL(td3_norm_kernel, dim3(T_NB, 1 + lo.cost), dim3(256), 0, st, nr);
    TAdam ad = {lo.q.Pn, nq, B, dr->nslots, 0, Pc, (long)w.hstride, s->critic, s->critic_m, s->critic_v,
                actor_step ? s->critic_t : nullptr, stats, ws + w.gq, ws + w.rows, ws + w.ho[0][top], part,
                s->adam_step + 1, s->step, hp->lr_critic, hp->max_grad_norm, hp->critic_norm_coeff, hp->polyak,
                hp->one_minus_polyak, hp->beta1, hp->beta2, hp->adam_eps};
    hipLaunchKernelGGL(td3_adam_kernel, dim3(crr_blocks(lo.q.Pn, 256), nc), dim3(256), 0, st, ad);
    if (actor_step) {  // ddpg.py:498-547 with the UPDATED critic 1
      const CFwd pf = {s->actor, ws + w.xq, lo.ldsa, B, w.hp};
      if ((rc = crr_forward(lo.pi, &pf, 1, ws, st)) != OSA_OK) return rc;
      float* th = ws + w.hp[lo.pi.L - 1];
      hipLaunchKernelGGL(td3_pi_kernel, dim3(crr_blocks((long)B * lo.ldsa, 256)), dim3(256), 0, st, B, lo.A, lo.D, lo.lda,
                         lo.ldsa, th, ws + w.xq, ws + w.xc, ws + w.z[0][0]);
      if (!lag) {
        const CFwd qf = {s->critic, ws + w.xc, lo.ldsa, B, w.hq};
        if ((rc = crr_forward(lo.q, &qf, 1, ws, st)) != OSA_OK) return rc;
        if ((rc = td3_critic_dx(lo.q, s->critic, w.hq, w.z[0], w.dx, B, lo.ldsa, ws, st)) != OSA_OK) return rc;
        hipLaunchKernelGGL(td3_dpi_kernel, dim3(crr_blocks((long)B * lo.lda, 256)), dim3(256), 0, st, B, lo.A, lo.D,
                           lo.lda, lo.ldsa, ws + w.dx, th, ws + w.z[1][0]);
      } else {  // ddpg_lag.py:73-100: reward critic 0 and the cost critic, lambda read on the device
        const float* qc = s->critic + nq * Pc;
        const CFwd qf[2] = {{s->critic, ws + w.xc, lo.ldsa, B, w.hq}, {qc, ws + w.xc, lo.ldsa, B, x.hqc}};
        if ((rc = crr_forward(lo.q, qf, 2, ws, st)) != OSA_OK) return rc;
        hipLaunchKernelGGL(td3_lag_row_kernel, dim3(crr_blocks(B, 256)), dim3(256), 0, st, B, lag->multiplier,
                           ws + w.hq[top], ws + x.hqc[top], ws + w.z[0][0], ws + w.z[2][0], ws + x.nl);
        const bool gemm = lag->dact == OSA_TD3_LAG_DACT_GEMM;
        int cur = 0;
        if ((rc = td3_lag_critics_dx(lo, w, x, s->critic, gemm ? 1 : 0, ws, st, &cur)) != OSA_OK) return rc;
        if (gemm) {
          const TDact da = {{ws + w.z[0][cur], ws + w.z[2][cur]}, {s->critic + lo.q.oW[0], qc + lo.q.oW[0]}, th,
                            ws + x.dzpi, B, lo.A, lo.D, lo.q.out[0], lo.q.ldh[0], lo.q.ld[0], lo.lda};
          hipLaunchKernelGGL(td3_lag_dact_kernel, dim3((B + BC_ROWS - 1) / BC_ROWS), dim3(256), 0, st, da);
        } else {
          hipLaunchKernelGGL(td3_lag_dpi_kernel, dim3(crr_blocks((long)B * lo.lda, 256)), dim3(256), 0, st, B, lo.A,
                             lo.D, lo.lda, lo.ldsa, ws + w.dx, ws + x.dxc, th, ws + x.dzpi);
        }
      }
      const CBwd pb = {s->actor, ws + w.xq, lo.ldsa, w.hp, {lag ? x.dzpi : w.z[1][0], w.z[1][1]}, ws + w.gp};
      if ((rc = crr_backward(lo.pi, &pb, 1, B, ws, st)) != OSA_OK) return rc;
      double* apart = part + (long)2 * T_NB * 2;
      TNorm na = {{ws + w.gp, nullptr}, {s->actor, nullptr}, {lo.pi.P, 0}, {s->adam_step, nullptr}, apart, 0.f};
      hipLaunchKernelGGL(td3_norm_kernel, dim3(T_NB, 1), dim3(256), 0, st, na);
      TAdam aa = {lo.pi.Pn, 1, B, dr->nslots, 1, (long)lo.pi.P, 0, s->actor, s->actor_m, s->actor_v, s->actor_t, stats,
                  ws + w.gp, nullptr, ws + (lag ? x.nl : w.hq[top]), apart, s->adam_step, s->step, hp->lr_actor, hp->max_grad_norm, 0.f,
                  hp->polyak, hp->one_minus_polyak, hp->beta1, hp->beta2, hp->adam_eps};
      hipLaunchKernelGGL(td3_adam_kernel, dim3(crr_blocks(lo.pi.Pn, 256), 1), dim3(256), 0, st, aa);
    }
    hipLaunchKernelGGL(td3_finish_kernel, dim3(1), dim3(64), 0, st, s->step);
    OSA_CHECK_LAUNCH();
  }
  return OSA_OK;
}

int osa_td3_step(const osa_td3_desc* desc, const osa_td3_hparams* hp, const osa_td3_state* s, const osa_td3_ring* ring,
                 const osa_td3_draw_buffers* dr, float* stats, float* ws, size_t ws_floats, long update_count, int nsteps,
                 void* stream) {
  return td3_step_run(desc, hp, s, nullptr, ring, dr, stats, ws, ws_floats, update_count, nsteps, stream);
}

size_t osa_td3_lag_ws_floats(const osa_td3_desc* desc) {
  TLayout lo;
  if (td3_make_layout(desc, &lo) != OSA_OK || !lo.cost) return 0;
  return td3_lag_ws(lo, td3_ws(lo)).total;
}

size_t osa_td3_lag_dz_offset(const osa_td3_desc* desc) {
  TLayout lo;
  if (td3_make_layout(desc, &lo) != OSA_OK) return 0;
  return td3_lag_ws(lo, td3_ws(lo)).dzpi;
}

int osa_td3_lag_step(const osa_td3_desc* desc, const osa_td3_hparams* hp, const osa_td3_state* s, const osa_td3_lag* lag,
                     const osa_td3_ring* ring, const osa_td3_draw_buffers* dr, float* stats, float* ws, size_t ws_floats,
                     long update_count, int nsteps, void* stream) {
  OSA_REQUIRE(lag);
  return td3_step_run(desc, hp, s, lag, ring, dr, stats, ws, ws_floats, update_count, nsteps, stream);
}

int osa_td3_multiplier_update(const osa_td3_lag* lag, const float* carry, int ncarry, const float* ep_out, long ep_cap,
                              const long* ep_count, int update, float* stats, const long* step, int nslots,
                              void* stream) {
  OSA_REQUIRE(lag && lag->multiplier && lag->count && ep_out && ep_count && stats && step && nslots >= 1);
  OSA_REQUIRE(ncarry >= 0 && (ncarry == 0 || carry) && ep_cap >= 0 && lag->window_lens >= 1);
  if (lag->mode == OSA_TD3_LAG_ADAM) {
    OSA_REQUIRE(lag->adam && lag->lambda_lr >= 0.0);
  } else {
    OSA_REQUIRE(lag->mode == OSA_TD3_LAG_PID && lag->pid && lag->pid_d_delay >= 1 &&
                (reinterpret_cast<uintptr_t>(lag->pid) & 7) == 0);
  }
  TMult g = {*lag, carry, ep_out, ep_count, step, stats, ep_cap, ncarry, update, nslots};
  hipLaunchKernelGGL(td3_multiplier_kernel, dim3(1), dim3(64), 0, osa_stream(stream), g);
  OSA_CHECK_LAUNCH();
  return OSA_OK;
}

int osa_td3_act(const osa_td3_desc* desc, const float* actor, const float* obs, int ld_obs, long n, int mode, float noise,
                unsigned long long seed, unsigned long long offset, float* out, int ld_out, void* stream) {
  TLayout lo;
  OSA_REQUIRE(desc && out && n >= 1 && n <= 1024 && (mode == 0 || mode == 1) && noise >= 0.f);
  const int rc = td3_make_layout(desc, &lo);
  if (rc != OSA_OK) return rc;
  OSA_REQUIRE(ld_out >= lo.A && (mode == 1 || (actor && obs && ld_obs >= lo.D)));
  TAct g = {bcq_netk(lo.pi), actor, obs, out, lo.D, lo.A, ld_obs, ld_out, mode, noise, seed ^ TD3_KEY_ACT, offset};
  hipLaunchKernelGGL(td3_act_kernel, dim3((unsigned)n), dim3(256), 0, osa_stream(stream), g);
  OSA_CHECK_LAUNCH();
  return OSA_OK;
}

}  // extern "C"
