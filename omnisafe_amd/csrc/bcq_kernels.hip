// Offline BCQ and BCQ-Lag trained on the device from a device-resident dataset: replaces
// omnisafe/algorithms/offline/bcq.py:122-213, bcq_lag.py:91-193 and PerturbationActor.predict
// (models/actor/perturbation_actor.py:76-90) for the players.
//
// What makes a BCQ step expensive is its no-grad target chain: for every one of B S rows (256 x 10 at the YAML shape)
// decode a latent through the VAE decoder, perturb the action through the perturbation network and value it with both
// target critics -- four networks of four layers each, every layer waiting for the one before.  bcq_chain_kernel runs
// the whole chain in ONE launch:
//   * a workgroup of four waves owns 32 rows and carries them through every layer of every network; the activations
//     never leave the chip: two ping-pong LDS buffers [32][256 + 4] hold a layer's input and output, one LDS array
//     [32][obs || extra] holds the first-layer input of every network -- the observation columns are written once, the
//     columns behind them are z, then the decoded action, then the perturbed action, rewritten in place;
//   * rows come straight from the dataset through idx[slot][row / S]: no gather launch, no repeated copy of the S rows;
//   * weights skip LDS: every wave owns output columns of its own (tiles wave and wave + 4 of 32 columns, two
//     accumulators that share one activation fragment) and all waves share the 32 rows, so a staged weight would be read
//     once.  A lane loads W[n][k .. k + 3] with one 16-byte global load that feeds four float32 32x32x2 MFMAs (the K
//     permutation of gm_gemm.h), four K steps ahead of the MFMAs that consume them;
//   * a layer of at most 32 outputs (the heads: action, perturbation, q) splits K over the four waves instead; the
//     partial tiles meet in LDS and are added in wave order;
//   * bias, activation, tanh, a = act + phi tanh(.) and w min + (1 - w) max are fused into the accumulator write-back.
// Plain launch, no cooperative groups, no spin-waits, no atomics.  The same kernel stopped after the perturbation is
// the saved policy's predict.  The layer route (OSA_BCQ_ROUTE_LAYER) runs the same chain as one tile-GEMM launch per
// layer with small row kernels between the networks; it is the fallback for shapes the fused kernel does not take
// (a hidden width above 256, an observation too wide for the LDS budget) and the baseline it is measured against.
//
// Around the chain: the online critic pair's update (crr_layers.h: layer launches, Adam with the Polyak update fused
// in), the VAE update (osa_vae_step's launches on the same idx slot) and the perturbation network's update through
// critic 1's data gradient.  Every reduction has a fixed order; nothing in a step reads the host.
#include <math.h>

#include "chain_layer.h"

namespace {

struct BLayout {
  CNet enc, dec, pert, q;
  osa_vae_desc vd;
  int D, A, A2, B, S, pairs, ldsa, ldsz, lda, ldxin;
  long R;  // rows of the target chain: B S
};

int bcq_make_layout(const osa_bcq_desc* d, BLayout* lo) {
  if (!d) return OSA_EINVAL;
  if (d->obs_dim < 1 || d->obs_dim > 4096 || d->act_dim < 1) return OSA_EINVAL;
  if (d->batch < 1 || d->samples < 1 || d->pairs < 1 || d->pairs > 2) return OSA_EINVAL;
  if (d->act_dim > 32 || (long)d->batch * d->samples > (1l << 20)) return OSA_EUNSUPPORTED;
  for (int k = 0; k < 2; ++k)
    if (d->n_hidden[k] < 1 || d->n_hidden[k] + 1 > GM_MAXL) return OSA_EUNSUPPORTED;
  lo->D = d->obs_dim; lo->A = d->act_dim; lo->A2 = 2 * d->act_dim; lo->B = d->batch; lo->S = d->samples;
  lo->pairs = d->pairs;
  lo->ldsa = c4(lo->D + lo->A); lo->ldsz = c4(lo->D + lo->A2); lo->lda = c4(lo->A); lo->ldxin = lo->ldsz + 4;
  lo->R = (long)lo->B * lo->S;
  int width[GM_MAXL];
  const int na = d->n_hidden[0], nq = d->n_hidden[1];
  for (int l = 0; l < na; ++l) width[l] = d->hidden[0][l];
  int rc;
  width[na] = 2 * lo->A2;  // the VAE's two networks, as osa_vae_layout lays them out: encoder, then decoder
  if ((rc = crr_make_net(lo->enc, lo->D + lo->A, na + 1, width, d->activation[0], 2 * lo->A2, false)) != OSA_OK) return rc;
  width[na] = lo->A;
  if ((rc = crr_make_net(lo->dec, lo->D + lo->A2, na + 1, width, d->activation[0], lo->A, false)) != OSA_OK) return rc;
  if ((rc = crr_make_net(lo->pert, lo->D + lo->A, na + 1, width, d->activation[0], lo->A, false)) != OSA_OK) return rc;
  for (int l = 0; l < nq; ++l) width[l] = d->hidden[1][l];
  width[nq] = 1;
  if ((rc = crr_make_net(lo->q, lo->D + lo->A, nq + 1, width, d->activation[1], 1, false)) != OSA_OK) return rc;
  lo->vd = osa_vae_desc{};
  lo->vd.obs_dim = lo->D; lo->vd.act_dim = lo->A; lo->vd.n_hidden = na; lo->vd.activation = d->activation[0];
  lo->vd.batch = lo->B;
  for (int l = 0; l < na; ++l) lo->vd.hidden[l] = d->hidden[0][l];
  return OSA_OK;
}

// ---- the fused chain (its layer: chain_layer.h) ------------------------------------------------------------------
size_t bcq_chain_lds(const BLayout& lo) {
  return sizeof(float) * ((size_t)2 * BC_ROWS * BC_LDH + BC_PART + BC_ROWS * 32 + 2 * BC_ROWS + (size_t)BC_ROWS * lo.ldxin);
}
bool bcq_chain_ok(const BLayout& lo) {
  for (const CNet* n : {&lo.dec, &lo.pert, &lo.q})
    for (int l = 0; l + 1 < n->L; ++l)
      if (n->out[l] > BC_MAXW) return false;
  return bcq_chain_lds(lo) <= (size_t)BC_LDS_DYN;
}

// where the rows of a chain come from: row r is x[idx[slot][r / S]] (idx != null) or x[r], its latent z[slot][r]
struct BSrc {
  const float* x;
  const long* idx;   // [nslots][B]
  const long* step;  // null: slot 0
  const float* z;    // rows of ldz floats
  long nrows, z_slot;
  int ldx, ldz, nslots, B, S, M;
};
struct BChain {
  BSrc s;
  BNetK net[3];  // decoder, perturbation, critic
  const float *pdec, *ppert, *pq1, *pq2;
  float* out;    // stop: the perturbed action [M][ld_out]; else w min(q1, q2) + (1 - w) max(q1, q2) [M]
  int D, A, ldxin, stop, ld_out;
  float phi, w, omw;
};

__device__ __forceinline__ float bcq_mix(float q1, float q2, float w, float omw) {
  return __fadd_rn(__fmul_rn(w, fminf(q1, q2)), __fmul_rn(omw, fmaxf(q1, q2)));
}
__device__ __forceinline__ float bcq_perturb(float act, float phi, float pre) {
  return __fadd_rn(act, __fmul_rn(phi, gm_act(pre, OSA_ACT_TANH)));
}

__global__ __launch_bounds__(256) void bcq_chain_kernel(BChain g) {
  extern __shared__ __attribute__((aligned(16))) float bc_smem[];
  __shared__ BNetK nets[3];  // (a run-time layer index into the by-value argument would go through scratch memory)
  float* hb0 = bc_smem;
  float* hb1 = hb0 + BC_ROWS * BC_LDH;
  float* part = hb1 + BC_ROWS * BC_LDH;
  float* av = part + BC_PART;      // [32][32] the decoded action
  float* qv = av + BC_ROWS * 32;   // [2][32] the pair's values
  float* xin = qv + 2 * BC_ROWS;   // [32][ldxin] obs || z, then obs || act, then obs || a
  const int tid = threadIdx.x, m0 = blockIdx.x * BC_ROWS;
  const int D = g.D, A = g.A, ldxin = g.ldxin, M = g.s.M;
  if (tid == 0) {
    nets[0] = g.net[0];
    nets[1] = g.net[1];
    nets[2] = g.net[2];
  }
  const long slot = g.s.step ? *g.s.step % g.s.nslots : 0;
  const long* __restrict__ idx = g.s.idx ? g.s.idx + slot * g.s.B : nullptr;
  const float* __restrict__ z = g.s.z + slot * g.s.z_slot;
  for (int e = tid; e < BC_ROWS * ldxin; e += 256) {
    const int r = e / ldxin, c = e - r * ldxin, m = m0 + r;
    float v = 0.f;
    if (m < M) {
      if (c < D) {
        long gr = m;
        if (idx) {
          gr = idx[m / g.s.S];
          if (gr < 0 || gr >= g.s.nrows) gr = 0;  // (injected indices are checked on the host)
        }
        v = g.s.x[gr * g.s.ldx + c];
      } else if (c < D + 2 * A) {
        v = z[(long)m * g.s.ldz + (c - D)];
      }
    }
    xin[e] = v;
  }
  __syncthreads();
  const int lda4 = (D + A + 3) & ~3;
  // decoder: the action, kept for the perturbation and written behind the observation (padding zero)
  bc_net(&nets[0], g.pdec, xin, ldxin, hb0, hb1, part, [=](int row, int n, float v) {
    if (n < A) {
      av[row * 32 + n] = v;
      xin[row * ldxin + D + n] = v;
    } else if (D + n < lda4) {
      xin[row * ldxin + D + n] = 0.f;
    }
  });
  // perturbation: a = act + phi tanh(.)
  const float phi = g.phi;
  float* out = g.out;
  const int stop = g.stop, ld_out = g.ld_out;
  bc_net(&nets[1], g.ppert, xin, ldxin, hb0, hb1, part, [=](int row, int n, float v) {
    if (n < A) {
      const float a = bcq_perturb(av[row * 32 + n], phi, v);
      xin[row * ldxin + D + n] = a;
      if (stop && m0 + row < M) out[(long)(m0 + row) * ld_out + n] = a;
    }
  });
  if (stop) return;
  bc_net(&nets[2], g.pq1, xin, ldxin, hb0, hb1, part, [=](int row, int n, float v) {
    if (n == 0) qv[row] = v;
  });
  bc_net(&nets[2], g.pq2, xin, ldxin, hb0, hb1, part, [=](int row, int n, float v) {
    if (n == 0) qv[BC_ROWS + row] = v;
  });
  if (tid < BC_ROWS && m0 + tid < M) out[m0 + tid] = bcq_mix(qv[tid], qv[BC_ROWS + tid], g.w, g.omw);
}

int bcq_chain_launch(const BLayout& lo, const BSrc& s, const float* dec, const float* pert, const float* q1,
                     const float* q2, float phi, float w, float omw, float* out, int ld_out, int stop, hipStream_t st) {
  const size_t lds = bcq_chain_lds(lo);
  static OsaPerDeviceOnce attr_set;
  if (attr_set.need()) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&bcq_chain_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            BC_LDS_DYN) != hipSuccess)
      return OSA_EHIP;
    attr_set.set();
  }
  BChain g = {};
  g.s = s;
  g.net[0] = bcq_netk(lo.dec); g.net[1] = bcq_netk(lo.pert); g.net[2] = bcq_netk(lo.q);
  g.pdec = dec; g.ppert = pert; g.pq1 = q1; g.pq2 = q2; g.out = out;
  g.D = lo.D; g.A = lo.A; g.ldxin = lo.ldxin; g.stop = stop; g.ld_out = ld_out; g.phi = phi; g.w = w; g.omw = omw;
  hipLaunchKernelGGL(bcq_chain_kernel, dim3((s.M + BC_ROWS - 1) / BC_ROWS), dim3(256), lds, st, g);
  return hipGetLastError() == hipSuccess ? OSA_OK : OSA_EHIP;
}

// ---- the layer route's row kernels -------------------------------------------------------------------------------
struct BRowsWs {  // workspace of a chain over R rows (both routes: the fused one uses tq alone)
  size_t xz, xp, xc, hd[GM_MAXL], hp[GM_MAXL], hq[2][GM_MAXL], tq, zb, total;
};
BRowsWs bcq_rows_ws(const BLayout& lo, size_t R, size_t base) {
  BRowsWs w;
  size_t off = base;
  auto take = [&](size_t n) {
    const size_t o = off;
    off += (n + 3) / 4 * 4;
    return o;
  };
  w.xz = take(R * lo.ldsz); w.xp = take(R * lo.ldsa); w.xc = take(R * lo.ldsa);
  for (int l = 0; l < GM_MAXL; ++l) w.hd[l] = l < lo.dec.L ? take(R * lo.dec.ldh[l]) : 0;
  for (int l = 0; l < GM_MAXL; ++l) w.hp[l] = l < lo.pert.L ? take(R * lo.pert.ldh[l]) : 0;
  for (int k = 0; k < 2; ++k)
    for (int l = 0; l < GM_MAXL; ++l) w.hq[k][l] = l < lo.q.L ? take(R * lo.q.ldh[l]) : 0;
  w.tq = take(R);
  w.zb = take(R * lo.A2);  // predict's drawn latent
  w.total = off;
  return w;
}

// first-layer inputs of the three networks: xz = obs || z || 0, and the observation columns (and zero padding) of
// xp = obs || act and xc = obs || a, whose action columns the two kernels below fill
struct BRows {
  BSrc s;
  int D, A, ldsz, ldsa;
  float *xz, *xp, *xc;
};
__global__ __launch_bounds__(256) void bcq_rows_kernel(BRows g) {
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6), t = threadIdx.x & 63;
  if (m >= g.s.M) return;
  const long slot = g.s.step ? *g.s.step % g.s.nslots : 0;
  long gr = m;
  if (g.s.idx) {
    gr = g.s.idx[slot * g.s.B + m / g.s.S];
    if (gr < 0 || gr >= g.s.nrows) gr = 0;  // (injected indices are checked on the host)
  }
  const float* x = g.s.x + gr * g.s.ldx;
  const float* z = g.s.z + slot * g.s.z_slot + (long)m * g.s.ldz;
  for (int c = t; c < g.ldsz; c += 64)
    g.xz[(long)m * g.ldsz + c] = c < g.D ? x[c] : (c < g.D + 2 * g.A ? z[c - g.D] : 0.f);
  for (int c = t; c < g.ldsa; c += 64) {
    const float v = c < g.D ? x[c] : 0.f;
    g.xp[(long)m * g.ldsa + c] = v;
    g.xc[(long)m * g.ldsa + c] = v;
  }
}
// mode 0: xp[m][D + j] = act[m][j] (the decoder's output).  mode 1: xc[m][D + j] = act + phi tanh(pre[m][j]); pre is
// overwritten with the tanh (the actor step's backward reads it); out != null: the perturbed action of predict
__global__ __launch_bounds__(256) void bcq_action_kernel(int mode, int M, int A, int D, int lda, int ldsa,
                                                         const float* __restrict__ act, float* __restrict__ pre,
                                                         float* __restrict__ x, float phi, float* __restrict__ out,
                                                         int ld_out) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)M * A) return;
  const long m = e / A;
  const int j = (int)(e - m * A);
  float v = act[m * lda + j];
  if (mode == 1) {
    const float p = pre[m * lda + j];
    v = bcq_perturb(v, phi, p);
    pre[m * lda + j] = gm_act(p, OSA_ACT_TANH);
    if (out) out[m * ld_out + j] = v;
  }
  x[m * ldsa + D + j] = v;
}
__global__ __launch_bounds__(256) void bcq_mix_kernel(int M, const float* __restrict__ q1, const float* __restrict__ q2,
                                                      float w, float omw, float* __restrict__ out) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m < M) out[m] = bcq_mix(q1[4 * m], q2[4 * m], w, omw);
}

// decoder and perturbation over the rows of `s`, layer by layer: leaves xc = obs || a, the activations of both networks
// (the perturbation head holding its tanh) and, with out, the perturbed action
int bcq_actor_layers(const BLayout& lo, const BSrc& s, const float* dec, const float* pert, float phi, float* ws,
                     const BRowsWs& w, float* out, int ld_out, hipStream_t st) {
  const int M = s.M;
  BRows ro = {s, lo.D, lo.A, lo.ldsz, lo.ldsa, ws + w.xz, ws + w.xp, ws + w.xc};
  hipLaunchKernelGGL(bcq_rows_kernel, dim3(crr_blocks(M, 4)), dim3(256), 0, st, ro);
  int rc;
  const CFwd df = {dec, ws + w.xz, lo.ldsz, M, w.hd};
  if ((rc = crr_forward(lo.dec, &df, 1, ws, st)) != OSA_OK) return rc;
  float* act = ws + w.hd[lo.dec.L - 1];
  hipLaunchKernelGGL(bcq_action_kernel, dim3(crr_blocks((long)M * lo.A, 256)), dim3(256), 0, st, 0, M, lo.A, lo.D, lo.lda,
                     lo.ldsa, act, (float*)nullptr, ws + w.xp, 0.f, (float*)nullptr, 0);
  const CFwd pf = {pert, ws + w.xp, lo.ldsa, M, w.hp};
  if ((rc = crr_forward(lo.pert, &pf, 1, ws, st)) != OSA_OK) return rc;
  hipLaunchKernelGGL(bcq_action_kernel, dim3(crr_blocks((long)M * lo.A, 256)), dim3(256), 0, st, 1, M, lo.A, lo.D, lo.lda,
                     lo.ldsa, act, ws + w.hp[lo.pert.L - 1], ws + w.xc, phi, out, ld_out);
  return OSA_OK;
}

// the chain's values tq[M] on either route
int bcq_chain(const BLayout& lo, int route, const BSrc& s, const float* dec, const float* pert, const float* q1,
              const float* q2, float phi, float wmin, float omw, float* ws, const BRowsWs& w, hipStream_t st) {
  if (route == OSA_BCQ_ROUTE_FUSED)
    return bcq_chain_launch(lo, s, dec, pert, q1, q2, phi, wmin, omw, ws + w.tq, 0, 0, st);
  int rc;
  if ((rc = bcq_actor_layers(lo, s, dec, pert, phi, ws, w, nullptr, 0, st)) != OSA_OK) return rc;
  const CFwd qf[2] = {{q1, ws + w.xc, lo.ldsa, s.M, w.hq[0]}, {q2, ws + w.xc, lo.ldsa, s.M, w.hq[1]}};
  if ((rc = crr_forward(lo.q, qf, 2, ws, st)) != OSA_OK) return rc;
  const int top = lo.q.L - 1;
  hipLaunchKernelGGL(bcq_mix_kernel, dim3(crr_blocks(s.M, 256)), dim3(256), 0, st, s.M, ws + w.hq[0][top],
                     ws + w.hq[1][top], wmin, omw, ws + w.tq);
  return OSA_OK;
}

// ---- the step's own workspace and kernels ------------------------------------------------------------------------
struct BWs {
  BRowsWs r;
  size_t xq, rcd, ho[2][GM_MAXL], z[2][2], dx[2], gq, gp, vae, total;
};
BWs bcq_ws(const BLayout& lo) {
  BWs w;
  w.r = bcq_rows_ws(lo, (size_t)lo.R, 0);
  size_t off = w.r.total;
  auto take = [&](size_t n) {
    const size_t o = off;
    off += (n + 3) / 4 * 4;
    return o;
  };
  const size_t B = lo.B;
  w.xq = take(B * lo.ldsa);
  w.rcd = take(3 * B);
  for (int k = 0; k < 2; ++k)
    for (int l = 0; l < GM_MAXL; ++l) w.ho[k][l] = l < lo.q.L ? take(B * lo.q.ldh[l]) : 0;
  const int mz = lo.pert.maxldh > lo.q.maxldh ? lo.pert.maxldh : lo.q.maxldh;
  for (int k = 0; k < 2; ++k)
    for (int j = 0; j < 2; ++j) w.z[k][j] = take(B * mz);
  for (int k = 0; k < 2; ++k) w.dx[k] = take(B * lo.ldsa);
  w.gq = take((size_t)2 * lo.q.P);
  w.gp = take(lo.pert.P);
  w.vae = take(osa_vae_ws_floats(&lo.vd));
  w.total = off;
  return w;
}

#define BCQ_KEY_IDX 0x42435149445831ull /* keys of their own: seed ^ key, counter = (step, element) */
#define BCQ_KEY_ZR 0x4243515A523031ull
#define BCQ_KEY_ZC 0x4243515A433031ull
#define BCQ_KEY_EPS 0x42435145505331ull
#define BCQ_KEY_ZA 0x4243515A413031ull

// idx[slot][b]: 64 random bits, multiply-high into [0, N)
__global__ __launch_bounds__(256) void bcq_draw_idx_kernel(unsigned long long key, long first, int nsteps, int nslots,
                                                           int B, unsigned long long N, long* __restrict__ idx) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)nsteps * B) return;
  const long k = e / B, b = e - k * B, step = first + k;
  uint32_t w[4];
  osa_philox(key, (uint64_t)step, (uint64_t)b, w);
  const unsigned long long bits = (unsigned long long)w[0] | ((unsigned long long)w[1] << 32);
  idx[(step % nslots) * B + b] = (long)__umul64hi(bits, N);
}
// predict's latent: z[r][d] = the normal of Philox(seed, offset, r 2 A + d), evaluated in double and rounded once
__global__ __launch_bounds__(256) void bcq_draw_z_kernel(unsigned long long seed, unsigned long long offset, long n,
                                                         float* __restrict__ z) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  uint32_t w[4];
  osa_philox(seed, offset, (uint64_t)e, w);
  const double u1 = (double)osa_u01(w[0]), u2 = (double)osa_u01(w[1]);
  z[e] = (float)(sqrt(-2.0 * log(u1)) * cos(6.28318530717958647692 * u2));
}

// the data rows of the online pair: obs || act, and reward | cost | done
struct BGather {
  const float *obs, *act, *reward, *cost, *done;
  const long* idx;
  const long* step;
  long N;
  int ld_obs, ld_act, nslots, B, D, A, ldsa;
  float *xq, *rcd;
};
__global__ __launch_bounds__(256) void bcq_gather_kernel(BGather g) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), t = threadIdx.x & 63;
  if (b >= g.B) return;
  long i = g.idx[(*g.step % g.nslots) * g.B + b];
  if (i < 0 || i >= g.N) i = 0;  // (injected indices are checked on the host; never read outside the dataset)
  const float* o = g.obs + i * g.ld_obs;
  const float* a = g.act + i * g.ld_act;
  for (int c = t; c < g.ldsa; c += 64) g.xq[(long)b * g.ldsa + c] = c < g.D ? o[c] : (c < g.D + g.A ? a[c - g.D] : 0.f);
  if (t == 0) {
    g.rcd[b] = g.reward[i];
    g.rcd[g.B + b] = g.cost[i];
    g.rcd[2 * g.B + b] = g.done[i];
  }
}

// bcq.py:156-176 / bcq_lag.py:126-147: the max over a row's S chain values (the cost target takes the max too, as the
// reference writes it), y = signal + (1 - done) gamma max, both MSE losses, dL/dq, the first-row statistics
struct BTd {
  const float *q1, *q2;   // [B][4] the online pair on (obs, act)
  const float* tq;        // [B S] the chain's values
  const float *sig, *done;
  float *dz1, *dz2;       // [B][4]
  float* stats;
  const long* step;
  int* adam_step;
  int nslots, B, S, s_loss;
  float gamma;
};
__global__ __launch_bounds__(256) void bcq_td_kernel(BTd g) {
  __shared__ double red[17];
  double l1 = 0.0, l2 = 0.0;
  const float inv = 2.f / (float)g.B;
  float y0 = 0.f;
  for (int b = threadIdx.x; b < g.B; b += 256) {
    float qt = g.tq[(long)b * g.S];
    for (int s = 1; s < g.S; ++s) qt = fmaxf(qt, g.tq[(long)b * g.S + s]);
    const float y = __fadd_rn(g.sig[b], __fmul_rn(__fmul_rn(1.f - g.done[b], g.gamma), qt));
    const float e1 = g.q1[4 * b] - y, e2 = g.q2[4 * b] - y;
    l1 += (double)e1 * e1;
    l2 += (double)e2 * e2;
    const f32x4 d1 = {e1 * inv, 0.f, 0.f, 0.f}, d2 = {e2 * inv, 0.f, 0.f, 0.f};
    *reinterpret_cast<f32x4*>(g.dz1 + 4 * b) = d1;
    *reinterpret_cast<f32x4*>(g.dz2 + 4 * b) = d2;
    if (b == 0) y0 = y;
  }
  l1 = osa_block_sum<256>(l1, red);
  l2 = osa_block_sum<256>(l2, red);
  if (threadIdx.x == 0) {
    float* s = g.stats + (*g.step % g.nslots) * OSA_BCQ_NSTAT;
    s[g.s_loss] = (float)(l1 / g.B) + (float)(l2 / g.B);
    s[g.s_loss + 1] = g.q1[0];
    s[g.s_loss + 2] = y0;
    *g.adam_step += 1;
  }
}

// bcq.py:188-190 / bcq_lag.py:158-170: the actor loss -mean(q1r - lambda q1c) with lambda read before its update,
// dL/dq of critic 1 of each pair, the first-row statistics and (gate open) the Lagrange step on mean(q1c)
struct BActorLoss {
  const float *qr, *qc;  // [B][4]; qc null: BCQ
  float *dzr, *dzc;      // [B][4]
  float* lagrange;       // [4]: lambda, Adam m, v, step count
  float* stats;
  const long* step;
  int* adam_step;
  int nslots, B, open;
  float cost_limit, lambda_lr;
  double beta1, beta2, eps;
};
__global__ __launch_bounds__(256) void bcq_actor_loss_kernel(BActorLoss g) {
  __shared__ double red[17];
  const float lam = g.qc ? g.lagrange[0] : 0.f;
  const float invB = 1.f / (float)g.B;
  double sum = 0.0, sum_c = 0.0;
  for (int b = threadIdx.x; b < g.B; b += 256) {
    float v = g.qr[4 * b];
    const f32x4 dr = {-invB, 0.f, 0.f, 0.f};
    *reinterpret_cast<f32x4*>(g.dzr + 4 * b) = dr;
    if (g.qc) {
      const float c = g.qc[4 * b];
      v = __fsub_rn(v, __fmul_rn(lam, c));
      sum_c += (double)c;
      const f32x4 dc = {lam * invB, 0.f, 0.f, 0.f};
      *reinterpret_cast<f32x4*>(g.dzc + 4 * b) = dc;
    }
    sum += (double)v;
  }
  sum = osa_block_sum<256>(sum, red);  // (its barriers: every thread has read lambda before thread 0 steps it)
  sum_c = osa_block_sum<256>(sum_c, red);
  if (threadIdx.x == 0) {
    float* s = g.stats + (*g.step % g.nslots) * OSA_BCQ_NSTAT;
    s[9] = (float)(-sum / g.B);
    s[10] = g.qr[0];
    *g.adam_step += 1;
    if (g.qc) {
      s[11] = g.qc[0];
      float l = lam;
      if (g.open) {  // common/lagrange.py: one Adam step on -lambda (Jc - cost_limit), then lambda <- max(lambda, 0)
        const float grad = -((float)(sum_c / g.B) - g.cost_limit);
        float mm = g.lagrange[1], vv = g.lagrange[2];
        const float t = g.lagrange[3] + 1.f;
        l = fmaxf(crr_adam1(grad, mm, vv, l, g.lambda_lr, g.beta1, g.beta2, g.eps, (int)t), 0.f);
        g.lagrange[0] = l;
        g.lagrange[1] = mm;
        g.lagrange[2] = vv;
        g.lagrange[3] = t;
      }
      s[12] = l;
    }
  }
}

// dL/d(perturbation pre-activation) = (dL/da of the reward critic + of the cost critic) phi (1 - tanh^2); padding zero
__global__ __launch_bounds__(256) void bcq_dpert_kernel(int B, int A, int D, int lda, int ldsa,
                                                        const float* __restrict__ dxr, const float* __restrict__ dxc,
                                                        const float* __restrict__ th, float phi, float* __restrict__ dz) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= B * lda) return;
  const int b = e / lda, j = e - b * lda;
  float d = 0.f;
  if (j < A) {
    float ga = dxr[(long)b * ldsa + D + j];
    if (dxc) ga += dxc[(long)b * ldsa + D + j];
    const float t = th[e];
    d = ga * phi * (1.f - t * t);
  }
  dz[e] = d;
}

// the step's last launch: the VAE's losses join the row, the step counter advances -- nothing after this reads the slot
__global__ void bcq_finish_kernel(const float* __restrict__ vae_stats, float* __restrict__ stats, long* step, int nslots) {
  if (threadIdx.x != 0) return;
  const long slot = *step % nslots;
  for (int k = 0; k < 3; ++k) stats[slot * OSA_BCQ_NSTAT + k] = vae_stats[slot * OSA_VAE_NSTAT + k];
  *step += 1;
}

// the data gradient of up to two critics down to their input rows: dx[j][B][ldsa] = dL/d(obs || a)
int bcq_critic_dx(const CNet& n, const float* const* params, const size_t* const* h, const size_t (*z)[2],
                  const size_t* dx, int njob, int B, int ldsa, float* ws, hipStream_t st) {
  int cur = 0;
  for (int l = n.L - 1; l >= 0; --l) {
    GArgs gd = {};
    gd.splits = 1;
    for (int j = 0; j < njob; ++j) {
      GProb q = crr_prob();  // dZ_{l-1}[rows][in] = (dZ_l[rows][out] . W_l[out][in]) * act'(H_{l-1})
      q.A = ws + z[j][cur]; q.lda = n.ldh[l];
      q.B = params[j] + n.oW[l]; q.ldb = n.ld[l];
      q.M = B; q.N = n.in[l]; q.K = n.out[l];
      if (l > 0) {
        q.C = ws + z[j][cur ^ 1]; q.ldc = n.ldh[l - 1];
        q.dact = n.act; q.aux = ws + h[j][l - 1]; q.ldaux = n.ldh[l - 1];
      } else {
        q.C = ws + dx[j]; q.ldc = ldsa;
      }
      gd.p[gd.nprob++] = q;
    }
    const int rc = gm_gemm<false, true>(gd, st);
    if (rc != OSA_OK) return rc;
    cur ^= 1;
  }
  return OSA_OK;
}

int bcq_route_ok(const BLayout& lo, int route) {
  if (route != OSA_BCQ_ROUTE_LAYER && route != OSA_BCQ_ROUTE_FUSED) return OSA_EINVAL;
  return route == OSA_BCQ_ROUTE_FUSED && !bcq_chain_ok(lo) ? OSA_EUNSUPPORTED : OSA_OK;
}

}  // namespace

extern "C" {

int osa_bcq_layout(const osa_bcq_desc* desc, int* out) {
  BLayout lo;
  OSA_REQUIRE(desc && out);
  const int rc = bcq_make_layout(desc, &lo);
  if (rc != OSA_OK) return rc;
  out[0] = lo.enc.P; out[1] = lo.dec.P; out[2] = lo.pert.P; out[3] = lo.q.P; out[4] = OSA_BCQ_NSTAT; out[5] = 0;
  int k = 6;
  for (int net = 0; net < 2; ++net) {
    const CNet& n = net == 0 ? lo.pert : lo.q;
    for (int l = 0; l < OSA_GMLP_MAX_LAYERS; ++l) {
      out[k++] = l < n.L ? n.oW[l] : -1;
      out[k++] = l < n.L ? n.ob[l] : -1;
      out[k++] = l < n.L ? n.ld[l] : 0;
    }
  }
  return OSA_OK;
}

size_t osa_bcq_ws_floats(const osa_bcq_desc* desc) {
  BLayout lo;
  if (bcq_make_layout(desc, &lo) != OSA_OK) return 0;
  return bcq_ws(lo).total;
}

int osa_bcq_chain_supported(const osa_bcq_desc* desc) {
  BLayout lo;
  return bcq_make_layout(desc, &lo) == OSA_OK && bcq_chain_ok(lo) ? 1 : 0;
}

int osa_bcq_draws(const osa_bcq_desc* desc, unsigned long long seed, long first_step, int nsteps, int nslots,
                  long n_rows, long* idx, float* z_r, float* z_c, float* eps, float* z_a, void* stream) {
  BLayout lo;
  OSA_REQUIRE(desc && idx && z_r && eps && z_a);
  const int rc = bcq_make_layout(desc, &lo);
  if (rc != OSA_OK) return rc;
  OSA_REQUIRE(first_step >= 0 && nsteps >= 1 && nslots >= 1 && nsteps <= nslots && n_rows >= 1);
  OSA_REQUIRE(lo.pairs == 1 || z_c);
  hipStream_t st = osa_stream(stream);
  hipLaunchKernelGGL(bcq_draw_idx_kernel, dim3(crr_blocks((long)nsteps * lo.B, 256)), dim3(256), 0, st,
                     seed ^ BCQ_KEY_IDX, first_step, nsteps, nslots, lo.B, (unsigned long long)n_rows, idx);
  const long pb = (long)lo.B * lo.A2, pr = lo.R * lo.A2;
  auto normals = [&](unsigned long long key, long per, float* dst) {
    hipLaunchKernelGGL(crr_draw_eps_kernel, dim3(crr_blocks(nsteps * per, 256)), dim3(256), 0, st, seed ^ key,
                       first_step, nsteps, nslots, per, dst);
  };
  normals(BCQ_KEY_ZR, pr, z_r);
  if (lo.pairs == 2) normals(BCQ_KEY_ZC, pr, z_c);
  normals(BCQ_KEY_EPS, pb, eps);
  normals(BCQ_KEY_ZA, pb, z_a);
  OSA_CHECK_LAUNCH();
  return OSA_OK;
}

int osa_bcq_target_q(const osa_bcq_desc* desc, const osa_bcq_hparams* hp, const osa_bcq_state* s,
                     const osa_crr_data* data, const long* idx, int nslots, int pair, const float* z, float* out,
                     float* ws, size_t ws_floats, void* stream) {
  BLayout lo;
  OSA_REQUIRE(desc && hp && s && data && idx && z && out && ws && nslots >= 1);
  int rc = bcq_make_layout(desc, &lo);
  if (rc != OSA_OK) return rc;
  if ((rc = bcq_route_ok(lo, hp->route)) != OSA_OK) return rc;
  OSA_REQUIRE(pair >= 0 && pair < lo.pairs && s->vae && s->pert && s->target && s->step && data->next_obs);
  OSA_REQUIRE(data->n_rows >= 1 && data->ld_next >= lo.D);
  const BWs w = bcq_ws(lo);
  OSA_REQUIRE(ws_floats >= w.total && (reinterpret_cast<uintptr_t>(ws) & 15) == 0);
  hipStream_t st = osa_stream(stream);
  const BSrc src = {data->next_obs, idx, s->step, z, data->n_rows, 0, data->ld_next, lo.A2, nslots, lo.B, lo.S, (int)lo.R};
  const float* tg = s->target + (long)2 * pair * lo.q.P;
  if ((rc = bcq_chain(lo, hp->route, src, s->vae + lo.enc.P, s->pert, tg, tg + lo.q.P, hp->phi, hp->min_weight,
                      hp->one_minus_min_weight, ws, w.r, st)) != OSA_OK)
    return rc;
  if (hipMemcpyAsync(out, ws + w.r.tq, sizeof(float) * lo.R, hipMemcpyDeviceToDevice, st) != hipSuccess) return OSA_EHIP;
  OSA_CHECK_LAUNCH();
  return OSA_OK;
}

int osa_bcq_step(const osa_bcq_desc* desc, const osa_bcq_hparams* hp, const osa_bcq_state* s, const osa_crr_data* data,
                 const osa_bcq_draw_buffers* dr, float* stats, float* ws, size_t ws_floats, int nsteps, void* stream) {
  BLayout lo;
  OSA_REQUIRE(desc && hp && s && data && dr && stats && ws && nsteps >= 1);
  int rc = bcq_make_layout(desc, &lo);
  if (rc != OSA_OK) return rc;
  if ((rc = bcq_route_ok(lo, hp->route)) != OSA_OK) return rc;
  const BWs w = bcq_ws(lo);
  OSA_REQUIRE(ws_floats >= w.total && (reinterpret_cast<uintptr_t>(ws) & 15) == 0);
  OSA_REQUIRE(s->vae && s->vae_m && s->vae_v && s->pert && s->pert_m && s->pert_v && s->critic && s->critic_m &&
              s->critic_v && s->target && s->adam_step && s->step && s->vae_stats);
  OSA_REQUIRE(data->obs && data->act && data->reward && data->cost && data->next_obs && data->done && data->n_rows >= 1 &&
              data->ld_obs >= lo.D && data->ld_next >= lo.D && data->ld_act >= lo.A);
  OSA_REQUIRE(dr->idx && dr->z_r && dr->eps && dr->z_a && dr->nslots >= 1);
  const bool lag = lo.pairs == 2;
  OSA_REQUIRE(!lag || (s->lagrange && dr->z_c));
  OSA_REQUIRE(hp->phi >= 0.f && hp->lr_actor >= 0.f && hp->lr_critic >= 0.f && hp->beta1 >= 0.0 && hp->beta1 < 1.0 &&
              hp->beta2 >= 0.0 && hp->beta2 < 1.0);
  for (const float* p : {s->vae, s->vae_m, s->vae_v, s->pert, s->pert_m, s->pert_v, s->critic, s->critic_m, s->critic_v,
                         s->target})
    OSA_REQUIRE((reinterpret_cast<uintptr_t>(p) & 15) == 0);
  hipStream_t st = osa_stream(stream);
  const int B = lo.B, top = lo.q.L - 1;
  const long Pc = lo.q.P;
  const float* dec = s->vae + lo.enc.P;
  const osa_vae_hparams vh = {hp->lr_actor, hp->vae_route, hp->beta1, hp->beta2, hp->adam_eps};
  const osa_vae_state vs = {s->vae, s->vae_m, s->vae_v, s->adam_step, s->step + 1};
  const osa_vae_draw_buffers vd = {dr->idx, dr->eps, dr->nslots};
  for (int it = 0; it < nsteps; ++it) {
    BGather ga = {data->obs, data->act, data->reward, data->cost, data->done, dr->idx, s->step, data->n_rows,
                  data->ld_obs, data->ld_act, dr->nslots, B, lo.D, lo.A, lo.ldsa, ws + w.xq, ws + w.rcd};
    hipLaunchKernelGGL(bcq_gather_kernel, dim3(crr_blocks(B, 4)), dim3(256), 0, st, ga);
    // ---- critic updates: the chain over next_obs with the pre-update actor and the pair's targets, then the pair
    for (int u = 0; u < lo.pairs; ++u) {
      float* on = s->critic + (long)2 * u * Pc;
      float* tg = s->target + (long)2 * u * Pc;
      const BSrc src = {data->next_obs, dr->idx, s->step, u == 0 ? dr->z_r : dr->z_c, data->n_rows, lo.R * lo.A2,
                        data->ld_next, lo.A2, dr->nslots, B, lo.S, (int)lo.R};
      if ((rc = bcq_chain(lo, hp->route, src, dec, s->pert, tg, tg + Pc, hp->phi, hp->min_weight,
                          hp->one_minus_min_weight, ws, w.r, st)) != OSA_OK)
        return rc;
      const CFwd cf[2] = {{on, ws + w.xq, lo.ldsa, B, w.ho[0]}, {on + Pc, ws + w.xq, lo.ldsa, B, w.ho[1]}};
      if ((rc = crr_forward(lo.q, cf, 2, ws, st)) != OSA_OK) return rc;
      BTd td = {ws + w.ho[0][top], ws + w.ho[1][top], ws + w.r.tq, ws + w.rcd + (size_t)u * B, ws + w.rcd + (size_t)2 * B,
                ws + w.z[0][0], ws + w.z[1][0], stats, s->step, s->adam_step + 2 + u, dr->nslots, B, lo.S, 3 + 3 * u,
                u == 0 ? hp->gamma : hp->cost_gamma};
      hipLaunchKernelGGL(bcq_td_kernel, dim3(1), dim3(256), 0, st, td);
      const CBwd cb[2] = {{on, ws + w.xq, lo.ldsa, w.ho[0], {w.z[0][0], w.z[0][1]}, ws + w.gq},
                          {on + Pc, ws + w.xq, lo.ldsa, w.ho[1], {w.z[1][0], w.z[1][1]}, ws + w.gq + Pc}};
      if ((rc = crr_backward(lo.q, cb, 2, B, ws, st)) != OSA_OK) return rc;
      // the target is not read again in this step: the Polyak update of bcq.py:205-213 rides on the pair's Adam
      hipLaunchKernelGGL(crr_adam_kernel, dim3(crr_blocks(lo.q.Pn, 256), 2), dim3(256), 0, st, lo.q.Pn, Pc, on,
                         s->critic_m + (long)2 * u * Pc, s->critic_v + (long)2 * u * Pc, ws + w.gq, Pc, tg,
                         s->adam_step + 2 + u, 1, hp->lr_critic, hp->beta1, hp->beta2, hp->adam_eps, hp->polyak,
                         hp->one_minus_polyak);
    }
    // ---- the VAE update: osa_vae_step's launches on the same slot, through a step counter of its own that its Adam
    // launch advances (equal to the step's between steps)
    if ((rc = osa_vae_step(&lo.vd, &vh, &vs, data, &vd, s->vae_stats, ws + w.vae, ws_floats - w.vae, 1, stream)) != OSA_OK)
      return rc;
    // ---- the actor update: the UPDATED VAE and critics on the data rows, a fresh latent
    const BSrc asrc = {data->obs, dr->idx, s->step, dr->z_a, data->n_rows, (long)B * lo.A2, data->ld_obs, lo.A2,
                       dr->nslots, B, 1, B};
    if ((rc = bcq_actor_layers(lo, asrc, dec, s->pert, hp->phi, ws, w.r, nullptr, 0, st)) != OSA_OK) return rc;
    const CFwd qf[2] = {{s->critic, ws + w.r.xc, lo.ldsa, B, w.r.hq[0]}, {s->critic + 2 * Pc, ws + w.r.xc, lo.ldsa, B, w.r.hq[1]}};
    if ((rc = crr_forward(lo.q, qf, lo.pairs, ws, st)) != OSA_OK) return rc;
    BActorLoss al = {ws + w.r.hq[0][top], lag ? ws + w.r.hq[1][top] : nullptr, ws + w.z[0][0], ws + w.z[1][0],
                     s->lagrange, stats, s->step, s->adam_step + 1, dr->nslots, B, hp->lagrange_open, hp->cost_limit,
                     hp->lambda_lr, hp->beta1, hp->beta2, hp->adam_eps};
    hipLaunchKernelGGL(bcq_actor_loss_kernel, dim3(1), dim3(256), 0, st, al);
    // critic 1's data gradient alone, down to the action columns (the reference's gradient into the VAE through `act`
    // is discarded by the next zero_grad: not computed)
    const float* qp[2] = {s->critic, s->critic + 2 * Pc};
    const size_t* qh[2] = {w.r.hq[0], w.r.hq[1]};
    if ((rc = bcq_critic_dx(lo.q, qp, qh, w.z, w.dx, lo.pairs, B, lo.ldsa, ws, st)) != OSA_OK) return rc;
    hipLaunchKernelGGL(bcq_dpert_kernel, dim3(crr_blocks((long)B * lo.lda, 256)), dim3(256), 0, st, B, lo.A, lo.D, lo.lda,
                       lo.ldsa, ws + w.dx[0], lag ? ws + w.dx[1] : (const float*)nullptr, ws + w.r.hp[lo.pert.L - 1],
                       hp->phi, ws + w.z[0][0]);
    const CBwd pb = {s->pert, ws + w.r.xp, lo.ldsa, w.r.hp, {w.z[0][0], w.z[0][1]}, ws + w.gp};
    if ((rc = crr_backward(lo.pert, &pb, 1, B, ws, st)) != OSA_OK) return rc;
    hipLaunchKernelGGL(crr_adam_kernel, dim3(crr_blocks(lo.pert.Pn, 256), 1), dim3(256), 0, st, lo.pert.Pn,
                       (long)lo.pert.P, s->pert, s->pert_m, s->pert_v, ws + w.gp, (long)lo.pert.P, (float*)nullptr,
                       s->adam_step + 1, 1, hp->lr_actor, hp->beta1, hp->beta2, hp->adam_eps, 0.f, 0.f);
    hipLaunchKernelGGL(bcq_finish_kernel, dim3(1), dim3(64), 0, st, s->vae_stats, stats, s->step, dr->nslots);
    OSA_CHECK_LAUNCH();
  }
  return OSA_OK;
}

size_t osa_bcq_predict_ws_floats(const osa_bcq_desc* desc, long n) {
  BLayout lo;
  if (n < 1 || n > (1l << 20) || bcq_make_layout(desc, &lo) != OSA_OK) return 0;
  return bcq_rows_ws(lo, (size_t)n, 0).total;
}

int osa_bcq_predict(const osa_bcq_desc* desc, int route, float phi, const float* decoder, const float* pert,
                    const float* obs, int ld_obs, const float* z, int ld_z, long n, unsigned long long seed,
                    unsigned long long offset, float* out, int ld_out, float* ws, size_t ws_floats, void* stream) {
  BLayout lo;
  OSA_REQUIRE(desc && decoder && pert && obs && out && ws && n >= 1);
  int rc = bcq_make_layout(desc, &lo);
  if (rc != OSA_OK) return rc;
  if (n > (1l << 20)) return OSA_EUNSUPPORTED;
  if ((rc = bcq_route_ok(lo, route)) != OSA_OK) return rc;
  OSA_REQUIRE(ld_obs >= lo.D && ld_out >= lo.A && (!z || ld_z >= lo.A2) && phi >= 0.f);
  const BRowsWs w = bcq_rows_ws(lo, (size_t)n, 0);
  OSA_REQUIRE(ws_floats >= w.total && (reinterpret_cast<uintptr_t>(ws) & 15) == 0);
  OSA_REQUIRE((reinterpret_cast<uintptr_t>(decoder) & 15) == 0 && (reinterpret_cast<uintptr_t>(pert) & 15) == 0);
  hipStream_t st = osa_stream(stream);
  if (!z) {  // vae_actor.py:95-96: a fresh standard-normal latent
    hipLaunchKernelGGL(bcq_draw_z_kernel, dim3(crr_blocks(n * lo.A2, 256)), dim3(256), 0, st, seed, offset, n * lo.A2,
                       ws + w.zb);
    z = ws + w.zb;
    ld_z = lo.A2;
  }
  const BSrc src = {obs, nullptr, nullptr, z, n, 0, ld_obs, ld_z, 1, (int)n, 1, (int)n};
  if (route == OSA_BCQ_ROUTE_FUSED)
    rc = bcq_chain_launch(lo, src, decoder, pert, nullptr, nullptr, phi, 0.f, 0.f, out, ld_out, 1, st);
  else
    rc = bcq_actor_layers(lo, src, decoder, pert, phi, ws, w, out, ld_out, st);
  if (rc != OSA_OK) return rc;
  OSA_CHECK_LAUNCH();
  return OSA_OK;
}

}  // extern "C"
