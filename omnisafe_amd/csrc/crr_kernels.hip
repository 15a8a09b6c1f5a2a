// Offline Critic Regularized Regression (CRR) and its constrained form (CCRR) trained on the device from a
// device-resident dataset: replaces omnisafe/algorithms/offline/crr.py:114-200, c_crr.py:91-206 and the batch sampling
// of omnisafe/common/offline/dataset.py:237-247.
//
// A 256 x 256 layer is 256 KB and does not fit the 160 KB LDS of a compute unit, so the step is layer-wise on the tile
// GEMM of general_mlp.hip (gm_gemm.h: exact float32 MFMA, up to three problems per launch) with small kernels around it:
//   draws     indices and both noise blocks of a whole block of steps, Philox keys of their own      osa_crr_draws
//   gather    dataset rows by index -> obs | next_obs rows of the actor, obs || act rows of the critics
//   rows      (next_obs, mu' + sigma eps) and (obs, mu + sigma eps_s) rows from ONE actor forward over obs | next_obs
//   td        min over the target pair, y, both MSE losses, dL/dq, first-row statistics
//   adam      Adam of one network group, the Polyak update of its target fused in
//   weight    min over the pair, mean over a row's S samples in index order, exp, clamp, lambda read; the Lagrange step
//   logp      weighted Gaussian log-likelihood: loss, dL/dmu, dL/dlog_std
//   finish    PolicyStd of the updated actor; the device step counter advances
// Every reduction has a fixed order (one workgroup, strided partial sums in double, wave shuffles, four waves added in
// order); no float atomics.  Nothing in a step reads the host: the draws' slot and the statistics row follow a device
// step counter, Adam's bias corrections device step counts, the multiplier lives in device memory -- a step captured
// into a single-stream graph advances on replay.
#include <math.h>

#include "gm_gemm.h"

namespace {

struct CNet {
  int L, in[GM_MAXL], out[GM_MAXL], ld[GM_MAXL], ldh[GM_MAXL], oW[GM_MAXL], ob[GM_MAXL];
  int oLS, Pn, P, act, maxldh;
};
struct CLayout {
  CNet a, q;
  int D, A, B, S, pairs, ldo, ldsa, lda;
  long R;  // rows of the critics' post-update forward: B data rows, then B S sampled rows
};

inline int c4(int x) { return (x + 3) / 4 * 4; }

int crr_make_net(CNet& n, int in_dim, int L, const int* width, int act, int out_dim, bool log_std) {
  if (L < 2 || L > GM_MAXL) return OSA_EUNSUPPORTED;  // at least one hidden layer
  if (act < OSA_ACT_TANH || act > OSA_ACT_IDENTITY) return OSA_EUNSUPPORTED;
  n.L = L;
  n.act = act;
  n.maxldh = 4;
  int off = 0, prev = in_dim;
  for (int l = 0; l < L; ++l) {
    const int w = width[l];
    if (w < 1 || w > 4096) return OSA_EINVAL;
    n.in[l] = prev; n.out[l] = w; n.ld[l] = c4(prev); n.ldh[l] = c4(w);
    if (n.ldh[l] > n.maxldh) n.maxldh = n.ldh[l];
    n.oW[l] = off; off += w * n.ld[l];
    n.ob[l] = off; off += c4(w);
    prev = w;
  }
  if (prev != out_dim) return OSA_EINVAL;
  n.oLS = off;
  if (log_std) off += c4(out_dim);
  n.Pn = off;
  n.P = (off + 15) / 16 * 16;
  return OSA_OK;
}

int crr_make_layout(const osa_crr_desc* d, CLayout* lo) {
  if (!d) return OSA_EINVAL;
  if (d->obs_dim < 1 || d->obs_dim > 4096 || d->act_dim < 1 || d->act_dim > 64) return OSA_EINVAL;
  if (d->batch < 1 || d->samples < 1 || d->pairs < 1 || d->pairs > 2) return OSA_EINVAL;
  if ((long)d->batch * (1 + (long)d->samples) > (1l << 20)) return OSA_EUNSUPPORTED;
  lo->D = d->obs_dim; lo->A = d->act_dim; lo->B = d->batch; lo->S = d->samples; lo->pairs = d->pairs;
  lo->ldo = c4(lo->D); lo->ldsa = c4(lo->D + lo->A); lo->lda = c4(lo->A);
  lo->R = (long)lo->B * (1 + lo->S);
  int rc = crr_make_net(lo->a, lo->D, d->n_layers[0], d->width[0], d->activation[0], lo->A, true);
  if (rc != OSA_OK) return rc;
  return crr_make_net(lo->q, lo->D + lo->A, d->n_layers[1], d->width[1], d->activation[1], 1, false);
}

struct CWs {
  size_t x2, ha[GM_MAXL], xq, xn[2], rcd, hq[4][GM_MAXL], ht[2][GM_MAXL], z[2][2], gq, ga, w, red, total;
};
CWs crr_ws(const CLayout& lo) {
  CWs w;
  size_t off = 0;
  auto take = [&](size_t n) {
    const size_t o = off;
    off += (n + 3) / 4 * 4;
    return o;
  };
  const size_t B = lo.B, R = lo.R;
  w.x2 = take(2 * B * lo.ldo);
  for (int l = 0; l < GM_MAXL; ++l) w.ha[l] = l < lo.a.L ? take(2 * B * lo.a.ldh[l]) : 0;
  w.xq = take(R * lo.ldsa);
  for (int p = 0; p < 2; ++p) w.xn[p] = take(B * lo.ldsa);
  w.rcd = take(3 * B);
  for (int k = 0; k < 4; ++k)
    for (int l = 0; l < GM_MAXL; ++l) w.hq[k][l] = (l < lo.q.L && k < 2 * lo.pairs) ? take(R * lo.q.ldh[l]) : 0;
  for (int k = 0; k < 2; ++k)
    for (int l = 0; l < GM_MAXL; ++l) w.ht[k][l] = l < lo.q.L ? take(B * lo.q.ldh[l]) : 0;
  const int mz = lo.a.maxldh > lo.q.maxldh ? lo.a.maxldh : lo.q.maxldh;
  for (int k = 0; k < 2; ++k)
    for (int j = 0; j < 2; ++j) w.z[k][j] = take(B * mz);
  w.gq = take((size_t)2 * lo.q.P);
  w.ga = take(lo.a.P);
  w.w = take(B);
  w.red = take(8);  // [0] mean over the batch of the sampled cost value (the Lagrange step's input)
  w.total = off;
  return w;
}

GProb crr_prob() {
  GProb p = {};
  p.splits = 1;
  p.act = -1;
  p.dact = -1;
  p.ones_n = -1;
  return p;
}

// ---- layers ------------------------------------------------------------------------------------------------------
struct CFwd {
  const float* params;  // the network's parameter block
  const float* X;       // input rows
  int ldx, M;
  const size_t* h;      // workspace offsets of its layer outputs
};
// forward of up to four networks of one shape, layer by layer: up to three networks per launch
int crr_forward(const CNet& n, const CFwd* job, int njob, float* ws, hipStream_t st) {
  for (int l = 0; l < n.L; ++l)
    for (int j0 = 0; j0 < njob; j0 += (njob == 4 ? 2 : 3)) {
      GArgs g = {};
      g.splits = 1;
      const int j1 = j0 + (njob == 4 ? 2 : 3) < njob ? j0 + (njob == 4 ? 2 : 3) : njob;
      for (int j = j0; j < j1; ++j) {
        GProb p = crr_prob();
        p.A = l == 0 ? job[j].X : ws + job[j].h[l - 1];
        p.lda = l == 0 ? job[j].ldx : n.ldh[l - 1];
        p.B = job[j].params + n.oW[l];
        p.ldb = n.ld[l];
        p.C = ws + job[j].h[l];
        p.ldc = n.ldh[l];
        p.M = job[j].M; p.N = n.out[l]; p.K = n.in[l];
        p.bias = job[j].params + n.ob[l];
        p.act = l + 1 < n.L ? n.act : -1;
        g.p[g.nprob++] = p;
      }
      const int rc = gm_gemm<false, false>(g, st);
      if (rc != OSA_OK) return rc;
    }
  return OSA_OK;
}

struct CBwd {
  const float* params;
  const float* X;
  int ldx;
  const size_t* h;
  size_t z[2];  // ping-pong dL/d(pre-activation); z[0] holds the top layer's on entry
  float* grad;  // the network's gradient block (parameter layout)
};
// backward of up to two networks of one shape over B rows: dW_l (+ db_l) straight into the gradient block (one split:
// K = B rows), then dZ of the layer below
int crr_backward(const CNet& n, const CBwd* job, int njob, int B, float* ws, hipStream_t st) {
  int cur = 0;
  for (int l = n.L - 1; l >= 0; --l) {
    GArgs gw = {}, gd = {};
    gw.splits = 1;
    gd.splits = 1;
    for (int j = 0; j < njob; ++j) {
      GProb p = crr_prob();  // dW_l[out][in] (+ db_l) = dZ_l^T [out][rows] . {H_{l-1}, 1}[rows][in + 1]
      p.A = ws + job[j].z[cur]; p.lda = n.ldh[l];
      p.B = l == 0 ? job[j].X : ws + job[j].h[l - 1];
      p.ldb = l == 0 ? job[j].ldx : n.ldh[l - 1];
      p.C = job[j].grad + n.oW[l]; p.ldc = n.ld[l];
      p.cb = job[j].grad + n.ob[l]; p.cb_pad = c4(n.out[l]);
      p.M = n.out[l]; p.N = n.in[l]; p.K = B;
      p.ones_n = n.in[l];
      gw.p[gw.nprob++] = p;
      if (l > 0) {  // dZ_{l-1}[rows][in] = (dZ_l[rows][out] . W_l[out][in]) * act'(H_{l-1})
        GProb q = crr_prob();
        q.A = ws + job[j].z[cur]; q.lda = n.ldh[l];
        q.B = job[j].params + n.oW[l]; q.ldb = n.ld[l];
        q.C = ws + job[j].z[cur ^ 1]; q.ldc = n.ldh[l - 1];
        q.M = B; q.N = n.in[l]; q.K = n.out[l];
        q.dact = n.act; q.aux = ws + job[j].h[l - 1]; q.ldaux = n.ldh[l - 1];
        gd.p[gd.nprob++] = q;
      }
    }
    int rc;
    if ((rc = gm_gemm<true, true>(gw, st)) != OSA_OK) return rc;
    if (gd.nprob > 0 && (rc = gm_gemm<false, true>(gd, st)) != OSA_OK) return rc;
    cur ^= 1;
  }
  return OSA_OK;
}

// ---- (a) draws ---------------------------------------------------------------------------------------------------
#define CRR_KEY_IDX 0x43525249445831ull   /* keys of their own: seed ^ key, counter = (step, element) */
#define CRR_KEY_NEXT 0x4352524E585431ull
#define CRR_KEY_NEXTC 0x4352524E584332ull
#define CRR_KEY_SAMP 0x43525253414D31ull

// idx[slot][b]: 64 random bits, multiply-high into [0, N)
__global__ __launch_bounds__(256) void crr_draw_idx_kernel(unsigned long long seed, long first, int nsteps, int nslots,
                                                           int B, unsigned long long N, long* __restrict__ idx) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)nsteps * B) return;
  const long k = e / B, b = e - k * B, step = first + k;
  uint32_t w[4];
  osa_philox(seed ^ CRR_KEY_IDX, (uint64_t)step, (uint64_t)b, w);
  const unsigned long long bits = (unsigned long long)w[0] | ((unsigned long long)w[1] << 32);
  idx[(step % nslots) * B + b] = (long)__umul64hi(bits, N);
}
// eps[slot][row][d]: the first Box-Muller normal of Philox(key, step, row A + d), key = seed ^ the buffer's constant
__global__ __launch_bounds__(256) void crr_draw_eps_kernel(unsigned long long key, long first, int nsteps, int nslots,
                                                           long per_step, float* __restrict__ eps) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)nsteps * per_step) return;
  const long k = e / per_step, i = e - k * per_step, step = first + k;
  uint32_t w[4];
  osa_philox(key, (uint64_t)step, (uint64_t)i, w);
  // osa_box_muller's first normal, evaluated in double and rounded once: a host restatement in float64 gives the same
  // float32 whatever the last bits of either side's log and cos (one launch per block of steps: off the step's path)
  const double u1 = (double)osa_u01(w[0]), u2 = (double)osa_u01(w[1]);
  eps[(step % nslots) * per_step + i] = (float)(sqrt(-2.0 * log(u1)) * cos(6.28318530717958647692 * u2));
}

// ---- (b) gather --------------------------------------------------------------------------------------------------
struct CGather {
  const float *obs, *act, *reward, *cost, *next_obs, *done;
  int ld_obs, ld_act, ld_next;
  long N;
  const long* idx;  // [nslots][B]
  const long* step;
  int nslots, B, D, A, ldo, ldsa;
  float *x2, *xq, *rcd;
};
__global__ __launch_bounds__(256) void crr_gather_kernel(CGather g) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), t = threadIdx.x & 63;
  if (b >= g.B) return;
  const long slot = *g.step % g.nslots;
  long i = g.idx[slot * g.B + b];
  if (i < 0 || i >= g.N) i = 0;  // (injected indices are checked on the host; never read outside the dataset)
  const float* o = g.obs + i * g.ld_obs;
  const float* no = g.next_obs + i * g.ld_next;
  const float* a = g.act + i * g.ld_act;
  float* xo = g.x2 + (long)b * g.ldo;
  float* xno = g.x2 + (long)(g.B + b) * g.ldo;
  float* xq = g.xq + (long)b * g.ldsa;
  for (int c = t; c < g.ldo; c += 64) {
    xo[c] = c < g.D ? o[c] : 0.f;
    xno[c] = c < g.D ? no[c] : 0.f;
  }
  for (int c = t; c < g.ldsa; c += 64) xq[c] = c < g.D ? o[c] : (c < g.D + g.A ? a[c - g.D] : 0.f);
  if (t == 0) {
    g.rcd[b] = g.reward[i];
    g.rcd[g.B + b] = g.cost[i];
    g.rcd[2 * g.B + b] = g.done[i];
  }
}

// the critics' input rows that carry an actor sample: (next_obs, mu(next_obs) + sigma eps_next) for every critic pair
// (a fresh draw each) and (obs, mu(obs) + sigma eps_samp[b, s]): the S repeated rows of an observation share one forward
struct CRows {
  const float *x2, *mu, *log_std;  // mu [2 B][lda]: obs rows, then next_obs rows
  const float* eps_next[2];
  const float* eps_samp;
  const long* step;
  int nslots, B, S, D, A, ldo, lda, ldsa, pairs;
  float* xn[2];
  float* xq;  // sampled rows start at row B
};
__global__ __launch_bounds__(256) void crr_rows_kernel(CRows g) {
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int t = threadIdx.x & 63;
  const long nrow = (long)g.B * (g.pairs + g.S);
  if (r >= nrow) return;
  const long slot = *g.step % g.nslots;
  const float *x, *mu, *eps;
  float* dst;
  if (r < (long)g.B * g.pairs) {
    const int p = (int)(r / g.B), b = (int)(r - (long)p * g.B);
    x = g.x2 + (long)(g.B + b) * g.ldo;
    mu = g.mu + (long)(g.B + b) * g.lda;
    eps = g.eps_next[p] + (slot * g.B + b) * g.A;
    dst = g.xn[p] + (long)b * g.ldsa;
  } else {
    const long q = r - (long)g.B * g.pairs;  // = b S + s
    const int b = (int)(q / g.S);
    x = g.x2 + (long)b * g.ldo;
    mu = g.mu + (long)b * g.lda;
    eps = g.eps_samp + (slot * g.B * g.S + q) * g.A;
    dst = g.xq + (g.B + q) * g.ldsa;
  }
  for (int c = t; c < g.ldsa; c += 64) {
    float v = 0.f;
    if (c < g.D) {
      v = x[c];
    } else if (c < g.D + g.A) {
      const int d = c - g.D;
      v = __fadd_rn(mu[d], __fmul_rn(expf(g.log_std[d]), eps[d]));  // Normal.rsample: loc + eps * scale
    }
    dst[c] = v;
  }
}

// ---- (c) TD target + MSE -----------------------------------------------------------------------------------------
struct CTd {
  const float *q1, *q2, *t1, *t2;  // [B][4] last-layer outputs: online pair on (obs, act), target pair on (next_obs, a')
  const float *sig, *done;         // reward or cost, done flags [B]
  float *dz1, *dz2;                // [B][4]
  float* stats;                    // [nslots][OSA_CRR_NSTAT]
  const long* step;
  int* adam_step;                  // this pair's Adam step count: incremented here, read by the Adam launch
  int nslots, B, s_loss, s_data, s_target;
  float gamma;
};
__global__ __launch_bounds__(256) void crr_td_kernel(CTd g) {
  __shared__ double red[17];
  double l1 = 0.0, l2 = 0.0;
  const float inv = 2.f / (float)g.B;
  float y0 = 0.f;
  for (int b = threadIdx.x; b < g.B; b += 256) {
    const float qt = fminf(g.t1[4 * b], g.t2[4 * b]);
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
    float* s = g.stats + (*g.step % g.nslots) * OSA_CRR_NSTAT;
    s[g.s_loss] = (float)(l1 / g.B) + (float)(l2 / g.B);
    s[g.s_data] = g.q1[0];
    s[g.s_target] = y0;
    *g.adam_step += 1;
  }
}

// ---- (f) Adam (+ Polyak) -----------------------------------------------------------------------------------------
// torch.optim.Adam's step on one element: the factors 1 - beta are the float32 roundings of the DOUBLE differences, as
// torch forms them (1.f - 0.999f is off by 1.3e-5 of itself), the bias corrections are taken in double; IEEE sqrt and
// division.  t: the step count, this step included.
__device__ __forceinline__ float crr_adam1(float g, float& m, float& v, float w, float lr, double beta1, double beta2,
                                           double eps, int t) {
  const float b2 = (float)beta2, omb1 = (float)(1.0 - beta1), omb2 = (float)(1.0 - beta2);
  m = fmaf(g - m, omb1, m);  // exp_avg.lerp_(grad, 1 - beta1)
  v = fmaf(g * g, omb2, v * b2);
  const float step_size = (float)((double)lr / (1.0 - pow(beta1, (double)t)));
  const float bc2_sqrt = (float)sqrt(1.0 - pow(beta2, (double)t));
  const float denom = sqrtf(v) / bc2_sqrt + (float)eps;
  return w - step_size * (m / denom);
}

// blockIdx.y = network of the group; adam = 0: the Polyak update alone (a target whose network took no step)
__global__ __launch_bounds__(256) void crr_adam_kernel(int Pn, long P, float* __restrict__ params, float* __restrict__ m,
                                                       float* __restrict__ v, const float* __restrict__ grad,
                                                       long grad_stride, float* __restrict__ target,
                                                       const int* __restrict__ adam_step, int adam, float lr,
                                                       double beta1, double beta2, double eps, float tau,
                                                       float one_minus_tau) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= Pn) return;
  const long o = (long)blockIdx.y * P + e;
  float w = params[o];
  if (adam) {
    float mm = m[o], vv = v[o];
    w = crr_adam1(grad[(long)blockIdx.y * grad_stride + e], mm, vv, w, lr, beta1, beta2, eps, *adam_step);
    params[o] = w;
    m[o] = mm;
    v[o] = vv;
  }
  if (target) target[o] = __fadd_rn(__fmul_rn(tau, w), __fmul_rn(one_minus_tau, target[o]));
}

// ---- (d) weight, (g) Lagrange step -------------------------------------------------------------------------------
struct CWeight {
  const float *qr1, *qr2;  // [R][4]: reward pair on the data rows, then the sampled rows
  const float *qc1, *qc2;  // cost pair on the data rows (CCRR)
  const float *sc1, *sc2;  // the pair that values the sampled rows for the cost advantage
  float* w;                // [B]
  float* lagrange;         // [4]: lambda, Adam m, v, step count
  float* stats;
  float* red;
  const long* step;
  int nslots, B, S, ccrr, open;
  float beta, cost_limit, lambda_lr;
  double beta1, beta2, eps;
};
__global__ __launch_bounds__(256) void crr_weight_kernel(CWeight g) {
  __shared__ double red[17];
  const float lam = g.ccrr ? g.lagrange[0] : 0.f;
  double sum_c = 0.0;
  for (int b = threadIdx.x; b < g.B; b += 256) {
    float sr = 0.f, sc = 0.f;
    for (int s = 0; s < g.S; ++s) {  // index order
      const long r = g.B + (long)b * g.S + s;
      sr += fminf(g.qr1[4 * r], g.qr2[4 * r]);
      if (g.ccrr) sc += fminf(g.sc1[4 * r], g.sc2[4 * r]);
    }
    const float adv_r = fminf(g.qr1[4 * b], g.qr2[4 * b]) - sr / (float)g.S;
    float w;
    if (g.ccrr) {
      const float mean_c = sc / (float)g.S;
      const float adv_c = fminf(g.qc1[4 * b], g.qc2[4 * b]) - mean_c;
      w = expf(__fsub_rn(adv_r, __fmul_rn(lam, adv_c)) / g.beta);
      w = fminf(fmaxf(w, 0.f), 1e10f);
      sum_c += (double)mean_c;
    } else {
      w = expf(adv_r / g.beta);
    }
    g.w[b] = w;
  }
  if (!g.ccrr) {
    if (threadIdx.x == 0) g.stats[(*g.step % g.nslots) * OSA_CRR_NSTAT + 7] = fminf(g.qr1[0], g.qr2[0]);
    return;
  }
  sum_c = osa_block_sum<256>(sum_c, red);
  if (threadIdx.x == 0) {
    float* s = g.stats + (*g.step % g.nslots) * OSA_CRR_NSTAT;
    s[7] = fminf(g.qr1[0], g.qr2[0]);
    s[8] = fminf(g.qc1[0], g.qc2[0]);
    const float jc = (float)(sum_c / g.B);
    g.red[0] = jc;
    float l = g.lagrange[0];
    if (g.open) {  // common/lagrange.py: one Adam step on -lambda (Jc - cost_limit), then lambda <- max(lambda, 0)
      const float grad = -(jc - g.cost_limit);
      float mm = g.lagrange[1], vv = g.lagrange[2];
      const float t = g.lagrange[3] + 1.f;
      l = crr_adam1(grad, mm, vv, l, g.lambda_lr, g.beta1, g.beta2, g.eps, (int)t);
      l = fmaxf(l, 0.f);
      g.lagrange[0] = l;
      g.lagrange[1] = mm;
      g.lagrange[2] = vv;
      g.lagrange[3] = t;
    }
    s[10] = l;
  }
}

// ---- (e) weighted Gaussian log-likelihood backward ---------------------------------------------------------------
struct CLogp {
  const float *mu, *xq, *log_std, *w;  // mu [B][lda] (rows of obs); the data action sits in xq[b][D ..]
  float* dz;                           // [B][lda]
  float* g_log_std;                    // [lda] of the actor's gradient block
  float* stats;
  const long* step;
  int* adam_step;
  int nslots, B, D, A, lda, ldsa;
};
__global__ __launch_bounds__(256) void crr_logp_kernel(CLogp g) {
  __shared__ double red[17];
  const float invB = 1.f / (float)g.B;
  double loss = 0.0;
  for (int b = threadIdx.x; b < g.B; b += 256) {
    const float wb = g.w[b];
    float lp = 0.f;
    for (int d = 0; d < g.lda; ++d) {
      float dz = 0.f;
      if (d < g.A) {
        const float sd = expf(g.log_std[d]), var = sd * sd;
        const float diff = g.xq[(long)b * g.ldsa + g.D + d] - g.mu[(long)b * g.lda + d];
        lp += -(diff * diff) / (2.f * var) - logf(sd) - 0.91893853320467274178f;
        dz = -(wb * invB) * diff / var;
      }
      g.dz[(long)b * g.lda + d] = dz;
    }
    loss += (double)wb * (double)(-lp);
  }
  loss = osa_block_sum<256>(loss, red);
  for (int d = 0; d < g.lda; ++d) {
    double acc = 0.0;
    if (d < g.A) {
      const float sd = expf(g.log_std[d]), var = sd * sd;
      for (int b = threadIdx.x; b < g.B; b += 256) {
        const float diff = g.xq[(long)b * g.ldsa + g.D + d] - g.mu[(long)b * g.lda + d];
        acc += (double)(g.w[b] * invB) * (1.0 - (double)(diff * diff / var));
      }
    }
    acc = osa_block_sum<256>(acc, red);
    if (threadIdx.x == 0) g.g_log_std[d] = (float)acc;
  }
  if (threadIdx.x == 0) {
    float* s = g.stats + (*g.step % g.nslots) * OSA_CRR_NSTAT;
    s[6] = (float)(loss / g.B);
    *g.adam_step += 1;
  }
}

// the step's last launch: PolicyStd of the UPDATED actor (crr.py:188 reads it after the optimiser step), then the step
// counter advances -- nothing after this reads the step's slot
__global__ void crr_finish_kernel(const float* __restrict__ log_std, int A, float* __restrict__ stats, long* step,
                                  int nslots) {
  if (threadIdx.x != 0) return;
  double sum = 0.0;
  for (int d = 0; d < A; ++d) sum += (double)expf(log_std[d]);
  stats[(*step % nslots) * OSA_CRR_NSTAT + 9] = (float)(sum / A);
  *step += 1;
}

unsigned crr_blocks(long n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

extern "C" {

int osa_crr_layout(const osa_crr_desc* desc, int* out) {
  CLayout lo;
  OSA_REQUIRE(desc && out);
  const int rc = crr_make_layout(desc, &lo);
  if (rc != OSA_OK) return rc;
  out[0] = lo.a.P; out[1] = lo.q.P; out[2] = lo.a.oLS; out[3] = OSA_CRR_NSTAT;
  int k = 4;
  for (int net = 0; net < 2; ++net) {
    const CNet& n = net == 0 ? lo.a : lo.q;
    for (int l = 0; l < OSA_GMLP_MAX_LAYERS; ++l) {
      out[k++] = l < n.L ? n.oW[l] : -1;
      out[k++] = l < n.L ? n.ob[l] : -1;
      out[k++] = l < n.L ? n.ld[l] : 0;
    }
  }
  return OSA_OK;
}

size_t osa_crr_ws_floats(const osa_crr_desc* desc) {
  CLayout lo;
  if (crr_make_layout(desc, &lo) != OSA_OK) return 0;
  return crr_ws(lo).total;
}

int osa_crr_draws(const osa_crr_desc* desc, unsigned long long seed, long first_step, int nsteps, int nslots,
                  long n_rows, long* idx, float* eps_next, float* eps_next_c, float* eps_samp, void* stream) {
  CLayout lo;
  OSA_REQUIRE(desc && idx && eps_next && eps_samp);
  const int rc = crr_make_layout(desc, &lo);
  if (rc != OSA_OK) return rc;
  OSA_REQUIRE(first_step >= 0 && nsteps >= 1 && nslots >= 1 && nsteps <= nslots && n_rows >= 1);
  OSA_REQUIRE(lo.pairs == 1 || eps_next_c);
  hipStream_t st = osa_stream(stream);
  hipLaunchKernelGGL(crr_draw_idx_kernel, dim3(crr_blocks((long)nsteps * lo.B, 256)), dim3(256), 0, st, seed, first_step,
                     nsteps, nslots, lo.B, (unsigned long long)n_rows, idx);
  const long pn = (long)lo.B * lo.A, ps = (long)lo.B * lo.S * lo.A;
  hipLaunchKernelGGL(crr_draw_eps_kernel, dim3(crr_blocks(nsteps * pn, 256)), dim3(256), 0, st, seed ^ CRR_KEY_NEXT,
                     first_step, nsteps, nslots, pn, eps_next);
  if (lo.pairs == 2)
    hipLaunchKernelGGL(crr_draw_eps_kernel, dim3(crr_blocks(nsteps * pn, 256)), dim3(256), 0, st, seed ^ CRR_KEY_NEXTC,
                       first_step, nsteps, nslots, pn, eps_next_c);
  hipLaunchKernelGGL(crr_draw_eps_kernel, dim3(crr_blocks(nsteps * ps, 256)), dim3(256), 0, st, seed ^ CRR_KEY_SAMP,
                     first_step, nsteps, nslots, ps, eps_samp);
  OSA_CHECK_LAUNCH();
  return OSA_OK;
}

int osa_crr_step(const osa_crr_desc* desc, const osa_crr_hparams* hp, const osa_crr_state* s, const osa_crr_data* data,
                 const osa_crr_draw_buffers* dr, float* stats, float* ws, size_t ws_floats, int nsteps, void* stream) {
  CLayout lo;
  OSA_REQUIRE(desc && hp && s && data && dr && stats && ws && nsteps >= 1);
  const int rc0 = crr_make_layout(desc, &lo);
  if (rc0 != OSA_OK) return rc0;
  const CWs w = crr_ws(lo);
  OSA_REQUIRE(ws_floats >= w.total && (reinterpret_cast<uintptr_t>(ws) & 15) == 0);
  OSA_REQUIRE(s->actor && s->actor_m && s->actor_v && s->critic && s->critic_m && s->critic_v && s->target &&
              s->adam_step && s->step);
  OSA_REQUIRE(data->obs && data->act && data->reward && data->cost && data->next_obs && data->done && data->n_rows >= 1 &&
              data->ld_obs >= lo.D && data->ld_next >= lo.D && data->ld_act >= lo.A);
  OSA_REQUIRE(dr->idx && dr->eps_next && dr->eps_samp && dr->nslots >= 1);
  const bool ccrr = lo.pairs == 2;
  OSA_REQUIRE(!ccrr || (s->lagrange && dr->eps_next_c));
  OSA_REQUIRE(hp->beta > 0.f && hp->lr_actor >= 0.f && hp->lr_critic >= 0.f && hp->beta1 >= 0.f && hp->beta1 < 1.f &&
              hp->beta2 >= 0.f && hp->beta2 < 1.f);
  for (const float* p : {s->actor, s->actor_m, s->actor_v, s->critic, s->critic_m, s->critic_v, s->target})
    OSA_REQUIRE((reinterpret_cast<uintptr_t>(p) & 15) == 0);
  hipStream_t st = osa_stream(stream);
  const int B = lo.B;
  const long Pc = lo.q.P;
  const bool refw = ccrr && hp->reference_wiring != 0;
  int rc;
  for (int it = 0; it < nsteps; ++it) {
    // ---- sample
    CGather ga = {};
    ga.obs = data->obs; ga.act = data->act; ga.reward = data->reward; ga.cost = data->cost;
    ga.next_obs = data->next_obs; ga.done = data->done; ga.ld_obs = data->ld_obs; ga.ld_act = data->ld_act;
    ga.ld_next = data->ld_next; ga.N = data->n_rows; ga.idx = dr->idx; ga.step = s->step; ga.nslots = dr->nslots;
    ga.B = B; ga.D = lo.D; ga.A = lo.A; ga.ldo = lo.ldo; ga.ldsa = lo.ldsa;
    ga.x2 = ws + w.x2; ga.xq = ws + w.xq; ga.rcd = ws + w.rcd;
    hipLaunchKernelGGL(crr_gather_kernel, dim3(crr_blocks(B, 4)), dim3(256), 0, st, ga);
    // ---- the actor over obs | next_obs: every sample of this step comes from this forward
    const CFwd af = {s->actor, ws + w.x2, lo.ldo, 2 * B, w.ha};
    if ((rc = crr_forward(lo.a, &af, 1, ws, st)) != OSA_OK) return rc;
    CRows ro = {};
    ro.x2 = ws + w.x2; ro.mu = ws + w.ha[lo.a.L - 1]; ro.log_std = s->actor + lo.a.oLS;
    ro.eps_next[0] = dr->eps_next; ro.eps_next[1] = dr->eps_next_c; ro.eps_samp = dr->eps_samp; ro.step = s->step;
    ro.nslots = dr->nslots; ro.B = B; ro.S = lo.S; ro.D = lo.D; ro.A = lo.A; ro.ldo = lo.ldo; ro.lda = lo.lda;
    ro.ldsa = lo.ldsa; ro.pairs = lo.pairs; ro.xn[0] = ws + w.xn[0]; ro.xn[1] = ws + w.xn[1]; ro.xq = ws + w.xq;
    hipLaunchKernelGGL(crr_rows_kernel, dim3(crr_blocks((long)B * (lo.pairs + lo.S), 4)), dim3(256), 0, st, ro);
    // ---- critic updates.  Intended wiring: pair u trains on signal u.  The reference's wiring (c_crr.py:103-133):
    // the second update trains the REWARD pair on the cost targets of the reward targets; the cost pair takes no step.
    for (int u = 0; u < lo.pairs; ++u) {
      const int pr = refw ? 0 : u;  // the pair this update trains
      float* on = s->critic + (long)2 * pr * Pc;
      float* tg = s->target + (long)2 * pr * Pc;
      const CFwd cf[4] = {{on, ws + w.xq, lo.ldsa, B, w.hq[2 * pr]},
                          {on + Pc, ws + w.xq, lo.ldsa, B, w.hq[2 * pr + 1]},
                          {tg, ws + w.xn[u], lo.ldsa, B, w.ht[0]},
                          {tg + Pc, ws + w.xn[u], lo.ldsa, B, w.ht[1]}};
      if ((rc = crr_forward(lo.q, cf, 4, ws, st)) != OSA_OK) return rc;
      const int top = lo.q.L - 1;
      CTd td = {};
      td.q1 = ws + w.hq[2 * pr][top]; td.q2 = ws + w.hq[2 * pr + 1][top];
      td.t1 = ws + w.ht[0][top]; td.t2 = ws + w.ht[1][top];
      td.sig = ws + w.rcd + (size_t)u * B; td.done = ws + w.rcd + (size_t)2 * B;
      td.dz1 = ws + w.z[0][0]; td.dz2 = ws + w.z[1][0]; td.stats = stats; td.step = s->step;
      td.adam_step = s->adam_step + 1 + pr; td.nslots = dr->nslots; td.B = B;
      td.s_loss = 3 * u; td.s_data = 3 * u + 1; td.s_target = 3 * u + 2; td.gamma = hp->gamma;
      hipLaunchKernelGGL(crr_td_kernel, dim3(1), dim3(256), 0, st, td);
      const CBwd cb[2] = {{on, ws + w.xq, lo.ldsa, w.hq[2 * pr], {w.z[0][0], w.z[0][1]}, ws + w.gq},
                          {on + Pc, ws + w.xq, lo.ldsa, w.hq[2 * pr + 1], {w.z[1][0], w.z[1][1]}, ws + w.gq + Pc}};
      if ((rc = crr_backward(lo.q, cb, 2, B, ws, st)) != OSA_OK) return rc;
      // the Polyak update rides on the pair's LAST Adam of the step (crr.py:192-200 runs it after every update)
      const bool last = !refw || u == lo.pairs - 1;
      hipLaunchKernelGGL(crr_adam_kernel, dim3(crr_blocks(lo.q.Pn, 256), 2), dim3(256), 0, st, lo.q.Pn, Pc, on,
                         s->critic_m + (long)2 * pr * Pc, s->critic_v + (long)2 * pr * Pc, ws + w.gq, Pc,
                         last ? tg : (float*)nullptr, s->adam_step + 1 + pr, 1, hp->lr_critic, hp->beta1, hp->beta2,
                         hp->adam_eps, hp->polyak, hp->one_minus_polyak);
    }
    if (refw)  // the untrained cost pair's target still takes its Polyak update (c_crr.py:197-206)
      hipLaunchKernelGGL(crr_adam_kernel, dim3(crr_blocks(lo.q.Pn, 256), 2), dim3(256), 0, st, lo.q.Pn, Pc,
                         s->critic + 2 * Pc, s->critic_m + 2 * Pc, s->critic_v + 2 * Pc, ws + w.gq, Pc, s->target + 2 * Pc,
                         s->adam_step + 2, 0, hp->lr_critic, hp->beta1, hp->beta2, hp->adam_eps, hp->polyak,
                         hp->one_minus_polyak);
    // ---- actor: the UPDATED critics on the data rows and the sampled rows
    CFwd pf[4];
    for (int k = 0; k < 2 * lo.pairs; ++k)
      pf[k] = CFwd{s->critic + (long)k * Pc, ws + w.xq, lo.ldsa, (int)lo.R, w.hq[k]};
    if ((rc = crr_forward(lo.q, pf, 2 * lo.pairs, ws, st)) != OSA_OK) return rc;
    const int top = lo.q.L - 1;
    CWeight we = {};
    we.qr1 = ws + w.hq[0][top]; we.qr2 = ws + w.hq[1][top];
    if (ccrr) {
      we.qc1 = ws + w.hq[2][top]; we.qc2 = ws + w.hq[3][top];
      we.sc1 = refw ? we.qr1 : we.qc1;  // c_crr.py:160-161 values the sampled rows with the reward pair
      we.sc2 = refw ? we.qr2 : we.qc2;
    }
    we.w = ws + w.w; we.lagrange = s->lagrange; we.stats = stats; we.red = ws + w.red; we.step = s->step;
    we.nslots = dr->nslots; we.B = B; we.S = lo.S; we.ccrr = ccrr; we.open = hp->lagrange_open; we.beta = hp->beta;
    we.cost_limit = hp->cost_limit; we.lambda_lr = hp->lambda_lr; we.beta1 = hp->beta1; we.beta2 = hp->beta2;
    we.eps = hp->adam_eps;
    hipLaunchKernelGGL(crr_weight_kernel, dim3(1), dim3(256), 0, st, we);
    CLogp lp = {};
    lp.mu = ws + w.ha[lo.a.L - 1]; lp.xq = ws + w.xq; lp.log_std = s->actor + lo.a.oLS; lp.w = ws + w.w;
    lp.dz = ws + w.z[0][0]; lp.g_log_std = ws + w.ga + lo.a.oLS; lp.stats = stats; lp.step = s->step;
    lp.adam_step = s->adam_step; lp.nslots = dr->nslots; lp.B = B; lp.D = lo.D; lp.A = lo.A; lp.lda = lo.lda;
    lp.ldsa = lo.ldsa;
    hipLaunchKernelGGL(crr_logp_kernel, dim3(1), dim3(256), 0, st, lp);
    const CBwd ab = {s->actor, ws + w.x2, lo.ldo, w.ha, {w.z[0][0], w.z[0][1]}, ws + w.ga};
    if ((rc = crr_backward(lo.a, &ab, 1, B, ws, st)) != OSA_OK) return rc;
    hipLaunchKernelGGL(crr_adam_kernel, dim3(crr_blocks(lo.a.Pn, 256), 1), dim3(256), 0, st, lo.a.Pn, (long)lo.a.P,
                       s->actor, s->actor_m, s->actor_v, ws + w.ga, (long)lo.a.P, (float*)nullptr, s->adam_step, 1,
                       hp->lr_actor, hp->beta1, hp->beta2, hp->adam_eps, 0.f, 0.f);
    hipLaunchKernelGGL(crr_finish_kernel, dim3(1), dim3(64), 0, st, s->actor + lo.a.oLS, lo.A, stats, s->step,
                       dr->nslots);
    OSA_CHECK_LAUNCH();
  }
  return OSA_OK;
}

}  // extern "C"
