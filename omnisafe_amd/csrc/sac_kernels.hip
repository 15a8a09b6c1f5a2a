// Off-policy SAC trained on the device from the replay ring of td3_kernels.hip: replaces omnisafe/algorithms/off_policy/
// sac.py:93-207 on ddpg.py:350-400 and GaussianSACActor.predict / log_prob.
//
// The step is TD3's chain of dependent launches (offpolicy_shared.h, crr_layers.h) plus the one thing TD3 has not: a
// stochastic actor whose top layer is [mean | log_std], 2 act_dim <= 64 columns wide.  Run as a layer it is a 6-column
// GEMM with a row kernel behind it on the way up, and a row kernel with two GEMMs behind it on the way down -- five
// launches around almost no arithmetic in a family that is bound by launches.  The fused head makes them two:
//   * sac_head_kernel (forward): a workgroup of four waves owns 32 rows.  The output columns are TWO float32 32x32x2
//     MFMA tiles, the means in one and the log-stds in the other, so that mu_j and log_std_j of a row sit at the same
//     accumulator position of the same lane: clamp, exp, the reparameterised sample, tanh and the per-element terms of
//     log pi need no shuffle.  K (the last hidden width) is split over the waves, operands straight from global memory;
//     the partial tiles meet in LDS and are added in wave order, the row sums of log pi in column order.  The write-back
//     puts a into the action columns of the critic input (tanh mu into a second input, log pi per row, and a, sigma eps
//     and the clamp mask for the backward, where asked).
//   * sac_head_grad_kernel (backward): workgroups own 128-column slabs of the last hidden width, a wave 32 columns.
//     Each workgroup recomputes the head's dz[B][2A] from the critics' dx and the saved values (cheap, and no exchange
//     between workgroups), walks the rows in 32-row tiles, accumulates dW[2A][slab] = dz^T H in registers over all rows
//     in a fixed order, and emits dH[rows][slab] = (dz W_top) act'(H) per tile; the first slab sums db.  No atomics.
// OSA_SAC_HEAD_LAYER runs the head as the layer and the row kernels: every shape, and the baseline.
#include <math.h>

#include "offpolicy_shared.h"

namespace {

struct SLayout {
  CNet pi, q;
  int D, A, B, cost, nc, ldsa, lda, ld2, K, ldk;
};

int sac_make_layout(const osa_sac_desc* d, SLayout* lo) {
  if (!d) return OSA_EINVAL;
  if (d->obs_dim < 1 || d->obs_dim > 4096 || d->act_dim < 1 || d->batch < 1) return OSA_EINVAL;
  if (d->use_cost < 0 || d->use_cost > 1) return OSA_EINVAL;
  if (d->act_dim > 32 || d->batch > (1 << 20)) return OSA_EUNSUPPORTED;
  for (int k = 0; k < 2; ++k)
    if (d->n_hidden[k] < 1 || d->n_hidden[k] + 1 > GM_MAXL) return OSA_EUNSUPPORTED;
  lo->D = d->obs_dim; lo->A = d->act_dim; lo->B = d->batch; lo->cost = d->use_cost;
  lo->nc = 2 + lo->cost;
  lo->ldsa = c4(lo->D + lo->A); lo->lda = c4(lo->A); lo->ld2 = c4(2 * lo->A);
  int width[GM_MAXL], rc;
  const int na = d->n_hidden[0], nq = d->n_hidden[1];
  for (int l = 0; l < na; ++l) width[l] = d->hidden[0][l];
  width[na] = 2 * lo->A;
  if ((rc = crr_make_net(lo->pi, lo->D, na + 1, width, d->activation[0], 2 * lo->A, false)) != OSA_OK) return rc;
  lo->K = lo->pi.in[na]; lo->ldk = lo->pi.ld[na];
  for (int l = 0; l < nq; ++l) width[l] = d->hidden[1][l];
  width[nq] = 1;
  return crr_make_net(lo->q, lo->D + lo->A, nq + 1, width, d->activation[1], 1, false);
}

bool sac_head_ok(const SLayout& lo) { return lo.K <= OSA_SAC_HEAD_MAX_WIDTH && lo.B <= OSA_SAC_HEAD_MAX_ROWS; }

// ---- the workspace -----------------------------------------------------------------------------------------------
struct SWs {
  size_t xq, xc, xn[2], rcd, ho[3][GM_MAXL], ht[3][GM_MAXL], hp[GM_MAXL], hq[2][GM_MAXL];
  size_t z[3][2], dx[2], gq, gp, rows, logp, nl, sa, sse, smask, part, hstride, total;
};
SWs sac_ws(const SLayout& lo) {
  SWs w = {};
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
  for (int j = 0; j < 3; ++j)
    for (int l = 0; l < GM_MAXL; ++l) w.ho[j][l] = l < lo.q.L ? take(B * lo.q.ldh[l]) : 0;
  w.hstride = w.ho[1][0] - w.ho[0][0];
  for (int j = 0; j < 3; ++j)
    for (int l = 0; l < GM_MAXL; ++l) w.ht[j][l] = l < lo.q.L ? take(B * lo.q.ldh[l]) : 0;
  for (int l = 0; l < GM_MAXL; ++l) w.hp[l] = l < lo.pi.L ? take(B * lo.pi.ldh[l]) : 0;
  for (int k = 0; k < 2; ++k)
    for (int l = 0; l < GM_MAXL; ++l) w.hq[k][l] = l < lo.q.L ? take(B * lo.q.ldh[l]) : 0;
  const int mz = lo.pi.maxldh > lo.q.maxldh ? lo.pi.maxldh : lo.q.maxldh;
  for (int j = 0; j < 3; ++j)
    for (int k = 0; k < 2; ++k) w.z[j][k] = take(B * mz);
  for (int k = 0; k < 2; ++k) w.dx[k] = take(B * lo.ldsa);
  w.gq = take((size_t)3 * lo.q.P);
  w.gp = take(lo.pi.P);
  w.rows = take(3 * B);
  w.logp = take(B);
  w.nl = take(4 * B);
  w.sa = take(B * lo.lda); w.sse = take(B * lo.lda); w.smask = take(B * lo.lda);
  w.part = take((size_t)3 * T_NB * 2 * 2);  // [group][T_NB][2] doubles
  w.total = off;
  return w;
}

// ---- the head's scalar algebra, shared by both routes and by osa_sac_act ---------------------------------------------
constexpr float S_LOG2 = 0.69314718055994531f, S_HALF_LOG_2PI = 0.91893853320467274f;

struct SHeadOut {
  float a, se, mask, term, tm;  // tanh u, sigma eps, 1[-20 < log_std < 2], the element's term of log pi, tanh mu
};
// gaussian_sac_actor.py:75-78, 96-99, 145-160: log_std clamped to [-20, 2], u = mu + sigma eps, a = tanh u and
// -eps^2 / 2 - log sigma - log(2 pi) / 2 - 2 (log 2 - u - softplus(-2 u))
__device__ __forceinline__ SHeadOut sac_head1(float mu, float lsr, float eps) {
  SHeadOut o;
  o.mask = (lsr > -20.f && lsr < 2.f) ? 1.f : 0.f;
  const float ls = fminf(fmaxf(lsr, -20.f), 2.f);
  o.se = __fmul_rn(expf(ls), eps);
  const float u = __fadd_rn(mu, o.se);
  o.a = gm_act(u, OSA_ACT_TANH);
  o.tm = gm_act(mu, OSA_ACT_TANH);
  const float x = -2.f * u;
  const float sp = fmaxf(x, 0.f) + log1pf(expf(-fabsf(x)));
  o.term = ((-0.5f * eps) * eps - ls - S_HALF_LOG_2PI) - 2.f * (S_LOG2 - u - sp);
  return o;
}
// g = dL/da, aB = alpha / B: dL/du = g (1 - a^2) + aB 2 a (the derivative of the squashing term of log pi is 2 tanh u);
// dL/dmu = dL/du, dL/dlog_std = (dL/du sigma eps - aB) inside the clamp
__device__ __forceinline__ void sac_dhead1(float g, float a, float se, float mask, float aB, float& dmu, float& dls) {
  const float du = g * (1.f - a * a) + aB * 2.f * a;
  dmu = du;
  dls = (du * se - aB) * mask;
}

struct SHead {
  const float *H, *W, *bias;  // fused: the last hidden layer's output [B][ldk], the top layer [2A][ldk], its bias
  const float* pre;           // layer: the top layer's output [B][ld2]
  const float* eps;           // [nslots][3][B][A]
  const long* step;
  const float* xsrc;          // non-null: the observation columns of xa are copied from these rows
  float *xa, *xb, *logp, *sa, *sse, *smask;  // each may be null
  int nslots, draw, B, A, D, ldk, ld2, ldsa, lda;
};

__device__ __forceinline__ void sac_head_store(const SHead& g, int m, int j, const SHeadOut& o) {
  if (g.xa) g.xa[(long)m * g.ldsa + g.D + j] = o.a;
  if (g.xb) g.xb[(long)m * g.ldsa + g.D + j] = o.tm;
  if (g.sa) {
    g.sa[(long)m * g.lda + j] = o.a;
    g.sse[(long)m * g.lda + j] = o.se;
    g.smask[(long)m * g.lda + j] = o.mask;
  }
}
__device__ __forceinline__ const float* sac_eps(const SHead& g) {
  return g.eps + ((*g.step % g.nslots) * 3 + g.draw) * (long)g.B * g.A;
}

// ---- the fused head, forward -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sac_head_kernel(SHead g) {
  __shared__ float part[2][4][16][64];  // tile (mean, log_std), wave, accumulator, lane
  __shared__ float term[BC_ROWS][33];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, kk = lane >> 5;
  const int m0 = blockIdx.x * BC_ROWS, A = g.A, B = g.B, ldk = g.ldk;
  const int nks = (ldk + 7) >> 3, per = (nks + 3) >> 2, s0 = wave * per, s1 = s0 + per < nks ? s0 + per : nks;
  const bool rok = m0 + l31 < B, cok = l31 < A;
  const float* hr = g.H + (long)(m0 + l31) * ldk + 4 * kk;
  const float* w0 = g.W + (long)l31 * ldk + 4 * kk;
  const float* w1 = g.W + (long)(A + l31) * ldk + 4 * kk;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x16 acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
  for (int s = s0; s < s1; ++s) {  // lane group kk consumes k = 8 s + 4 kk + q in MFMA step q
    const int k = 8 * s;
    const bool in = k + 4 * kk < ldk;
    const f32x4 af = (rok && in) ? *reinterpret_cast<const f32x4*>(hr + k) : zero;
    const f32x4 b0 = (cok && in) ? *reinterpret_cast<const f32x4*>(w0 + k) : zero;
    const f32x4 b1 = (cok && in) ? *reinterpret_cast<const f32x4*>(w1 + k) : zero;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(af[q], b0[q], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(af[q], b1[q], acc1, 0, 0, 0);
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    part[0][wave][r][lane] = acc0[r];
    part[1][wave][r][lane] = acc1[r];
  }
  if (g.xsrc)  // the critic input's observation columns and padding (the action columns: below)
    for (int e = tid; e < BC_ROWS * g.ldsa; e += 256) {
      const int r = e / g.ldsa, c = e - r * g.ldsa;
      if (m0 + r < B && (c < g.D || c >= g.D + A))
        g.xa[(long)(m0 + r) * g.ldsa + c] = c < g.D ? g.xsrc[(long)(m0 + r) * g.ldsa + c] : 0.f;
    }
  __syncthreads();
  const float* __restrict__ eps = sac_eps(g);
  const float bmu = cok ? g.bias[l31] : 0.f, bls = cok ? g.bias[A + l31] : 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {  // wave w adds accumulators 4 w .. 4 w + 3 of both tiles, in wave order
    const int r = 4 * wave + i, row = (r & 3) + 8 * (r >> 2) + 4 * kk, m = m0 + row;
    float mu = part[0][0][r][lane], ls = part[1][0][r][lane];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      mu += part[0][w][r][lane];
      ls += part[1][w][r][lane];
    }
    float t = 0.f;
    if (cok && m < B) {
      const SHeadOut o = sac_head1(mu + bmu, ls + bls, eps[(long)m * A + l31]);
      sac_head_store(g, m, l31, o);
      t = o.term;
    }
    term[row][l31] = t;
  }
  __syncthreads();
  if (tid < BC_ROWS && m0 + tid < B && g.logp) {
    float s = 0.f;
    for (int j = 0; j < A; ++j) s += term[tid][j];
    g.logp[m0 + tid] = s;
  }
}

// ---- the layer route's head: the same algebra on the top layer's output, four rows per workgroup --------------------
__global__ __launch_bounds__(256) void sac_head_row_kernel(SHead g) {
  __shared__ float term[4][32];
  const int w = threadIdx.x >> 6, j = threadIdx.x & 63, b = blockIdx.x * 4 + w;
  const bool ok = b < g.B;
  if (ok && g.xsrc)
    for (int c = j; c < g.ldsa; c += 64)
      if (c < g.D || c >= g.D + g.A) g.xa[(long)b * g.ldsa + c] = c < g.D ? g.xsrc[(long)b * g.ldsa + c] : 0.f;
  if (ok && j < g.A) {
    const float* pre = g.pre + (long)b * g.ld2;
    const SHeadOut o = sac_head1(pre[j], pre[g.A + j], sac_eps(g)[(long)b * g.A + j]);
    sac_head_store(g, b, j, o);
    term[w][j] = o.term;
  }
  __syncthreads();
  if (ok && j == 0 && g.logp) {
    float s = 0.f;
    for (int i = 0; i < g.A; ++i) s += term[w][i];
    g.logp[b] = s;
  }
}

// ---- TD targets with the entropy term; the actor loss's dq ---------------------------------------------------------------
struct STd {
  const float* q[3];   // [B][4] online critics
  const float* tq[3];  // [B][4] target critics
  const float *rcd, *logp, *log_alpha;
  float* dz[3];
  float* rows;
  int B, cost;
  float gamma;
};
__global__ __launch_bounds__(256) void sac_td_kernel(STd g) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= g.B) return;
  const float done = g.rcd[2 * g.B + b], inv2B = 2.f / (float)g.B, alpha = expf(*g.log_alpha);
  // sac.py:121-122: min(q1, q2) - log pi(a') alpha
  const float qm = __fsub_rn(fminf(g.tq[0][4 * b], g.tq[1][4 * b]), __fmul_rn(g.logp[b], alpha));
  const float yr = td3_y(g.rcd[b], done, g.gamma, qm);
  const float yc = g.cost ? td3_y(g.rcd[g.B + b], done, g.gamma, g.tq[2][4 * b]) : 0.f;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    if (j >= 2 + g.cost) break;
    const float e = g.q[j][4 * b] - (j < 2 ? yr : yc);
    const f32x4 d = {e * inv2B, 0.f, 0.f, 0.f};
    *reinterpret_cast<f32x4*>(g.dz[j] + 4 * b) = d;
    g.rows[(long)j * g.B + b] = e * e;
  }
}
// sac.py:207: mean(alpha log pi - min(q1, q2)): dq_k = -1 / B where critic k is the smaller one (critic 1 on a tie);
// nl[b][0] = min(q1, q2) - alpha log pi, whose negated mean the Adam launch writes as Loss/Loss_pi
__global__ __launch_bounds__(256) void sac_dq_kernel(int B, const float* __restrict__ q0, const float* __restrict__ q1,
                                                     const float* __restrict__ logp, const float* __restrict__ log_alpha,
                                                     float* __restrict__ dz0, float* __restrict__ dz1,
                                                     float* __restrict__ nl) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const float a = q0[4 * b], c = q1[4 * b], alpha = expf(*log_alpha), d = -1.f / (float)B;
  const bool first = a <= c;
  const f32x4 da = {first ? d : 0.f, 0.f, 0.f, 0.f}, dc = {first ? 0.f : d, 0.f, 0.f, 0.f};
  const f32x4 v = {__fsub_rn(first ? a : c, __fmul_rn(alpha, logp[b])), 0.f, 0.f, 0.f};
  *reinterpret_cast<f32x4*>(dz0 + 4 * b) = da;
  *reinterpret_cast<f32x4*>(dz1 + 4 * b) = dc;
  *reinterpret_cast<f32x4*>(nl + 4 * b) = v;
}

// ---- the head's gradient -----------------------------------------------------------------------------------------------
struct SGrad {
  const float *dx0, *dx1;         // [B][ldsa]: the two critics' dL/d(obs || a)
  const float *sa, *sse, *smask;  // [B][lda]: saved by the forward
  const float *H, *W;             // the last hidden layer's output [B][ldk], the top layer [2A][ldk]
  const float* log_alpha;
  float *gW, *gb, *dH, *dz;       // fused: the top layer's gradient blocks, dL/dZ of the last hidden layer; layer: dz
  int B, A, D, K, ldk, ld2, ldsa, lda, act;
};
// layer route: dz[B][ld2] = [dL/dmu | dL/dlog_std], padding zero
__global__ __launch_bounds__(256) void sac_dhead_row_kernel(SGrad g) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= g.B * g.ld2) return;
  const int b = e / g.ld2, c = e - b * g.ld2;
  float d = 0.f;
  if (c < 2 * g.A) {
    const int j = c < g.A ? c : c - g.A;
    const long x = (long)b * g.ldsa + g.D + j, s = (long)b * g.lda + j;
    float dmu, dls;
    sac_dhead1(g.dx0[x] + g.dx1[x], g.sa[s], g.sse[s], g.smask[s], expf(*g.log_alpha) / (float)g.B, dmu, dls);
    d = c < g.A ? dmu : dls;
  }
  g.dz[e] = d;
}

constexpr int SG_LD = 68;    // leading dimension of the dz tile: 64 columns [dmu | dlog_std], 16-byte aligned rows
constexpr int SG_SLAB = 128;  // hidden columns of a workgroup: 32 per wave
__global__ __launch_bounds__(256) void sac_head_grad_kernel(SGrad g) {
  __shared__ __attribute__((aligned(16))) float dzs[BC_ROWS][SG_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, kk = lane >> 5;
  const int A = g.A, B = g.B, ldk = g.ldk, n = blockIdx.x * SG_SLAB + 32 * wave + l31;
  const bool nok = n < g.K;
  const float aB = expf(*g.log_alpha) / (float)B;
  // the top layer's columns of this lane, for dH: element c of the dz tile's row pairs with W[c < 32 ? c : A + c - 32][n]
  float wf[8][4];
#pragma unroll
  for (int s = 0; s < 8; ++s)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = 8 * s + 4 * kk + q, j = c & 31;
      wf[s][q] = (nok && j < A) ? g.W[(long)(c < 32 ? j : A + j) * ldk + n] : 0.f;
    }
  f32x16 gmu, gls;
#pragma unroll
  for (int r = 0; r < 16; ++r) gmu[r] = gls[r] = 0.f;
  float db = 0.f;
  for (int m0 = 0; m0 < B; m0 += BC_ROWS) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {  // the tile's dz: 32 rows x 32 action columns, four elements per thread
      const int e = tid + 256 * i, row = e >> 5, j = e & 31, m = m0 + row;
      float dmu = 0.f, dls = 0.f;
      if (m < B && j < A) {
        const long x = (long)m * g.ldsa + g.D + j, s = (long)m * g.lda + j;
        sac_dhead1(g.dx0[x] + g.dx1[x], g.sa[s], g.sse[s], g.smask[s], aB, dmu, dls);
      }
      dzs[row][j] = dmu;
      dzs[row][32 + j] = dls;
    }
    __syncthreads();
    if (blockIdx.x == 0 && tid < 64)  // db: the rows in order
      for (int row = 0; row < BC_ROWS; ++row) db += dzs[row][tid];
    // dW[j][n] += sum over the tile's rows of dz[row][j] H[row][n]: lane group kk consumes row 8 s + 4 kk + q
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = 8 * s + 4 * kk + q, m = m0 + row;
        const float h = (nok && m < B) ? g.H[(long)m * ldk + n] : 0.f;
        gmu = __builtin_amdgcn_mfma_f32_32x32x2f32(dzs[row][l31], h, gmu, 0, 0, 0);
        gls = __builtin_amdgcn_mfma_f32_32x32x2f32(dzs[row][32 + l31], h, gls, 0, 0, 0);
      }
    // dH[row][n] = sum_c dz[row][c] W[c][n]
    f32x16 dh;
#pragma unroll
    for (int r = 0; r < 16; ++r) dh[r] = 0.f;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      if (((8 * s) & 31) >= A) continue;  // (uniform: columns past act_dim are zero on both sides)
      const f32x4 af = *reinterpret_cast<const f32x4*>(&dzs[l31][8 * s + 4 * kk]);
#pragma unroll
      for (int q = 0; q < 4; ++q) dh = __builtin_amdgcn_mfma_f32_32x32x2f32(af[q], wf[s][q], dh, 0, 0, 0);
    }
    if (n < ldk) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * kk;
        if (m < B) g.dH[(long)m * ldk + n] = nok ? dh[r] * gm_dact(g.H[(long)m * ldk + n], g.act) : 0.f;
      }
    }
    __syncthreads();  // the tile's dz is read: the next may be written
  }
  if (n < ldk) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = (r & 3) + 8 * (r >> 2) + 4 * kk;
      if (j < A) {
        g.gW[(long)j * ldk + n] = nok ? gmu[r] : 0.f;
        g.gW[(long)(A + j) * ldk + n] = nok ? gls[r] : 0.f;
      }
    }
  }
  if (blockIdx.x == 0 && tid < 64) {
    if ((tid & 31) < A) g.gb[(tid < 32 ? 0 : A) + (tid & 31)] = db;
    if (2 * A + tid < g.ld2) g.gb[2 * A + tid] = 0.f;  // padding of the bias block
  }
}

// the data gradients of BOTH reward critics down to their input rows, two problems per launch
int sac_critics_dx(const CNet& n, const float* params, const SWs& w, int B, int ldsa, float* ws, hipStream_t st) {
  int cur = 0;
  for (int l = n.L - 1; l >= 0; --l) {
    GArgs gd = {};
    gd.splits = 1;
    for (int k = 0; k < 2; ++k) {
      GProb q = crr_prob();  // dZ_{l-1}[rows][in] = (dZ_l[rows][out] . W_l[out][in]) * act'(H_{l-1})
      q.A = ws + w.z[k][cur]; q.lda = n.ldh[l];
      q.B = params + (long)k * n.P + n.oW[l]; q.ldb = n.ld[l];
      q.M = B; q.N = n.in[l]; q.K = n.out[l];
      if (l > 0) {
        q.C = ws + w.z[k][cur ^ 1]; q.ldc = n.ldh[l - 1];
        q.dact = n.act; q.aux = ws + w.hq[k][l - 1]; q.ldaux = n.ldh[l - 1];
      } else {
        q.C = ws + w.dx[k]; q.ldc = ldsa;
      }
      gd.p[gd.nprob++] = q;
    }
    const int rc = gm_gemm<false, true>(gd, st);
    if (rc != OSA_OK) return rc;
    cur ^= 1;
  }
  return OSA_OK;
}

// the actor on the rows X: its hidden layers on the tile GEMM, then the head on the route asked for
int sac_actor_forward(const SLayout& lo, const SWs& w, int head, const float* actor, const float* X, SHead g, float* ws,
                      hipStream_t st) {
  const CNet& n = lo.pi;
  const int top = n.L - 1;
  int rc;
  g.B = lo.B; g.A = lo.A; g.D = lo.D; g.ldk = lo.ldk; g.ld2 = lo.ld2; g.ldsa = lo.ldsa; g.lda = lo.lda;
  if (head == OSA_SAC_HEAD_LAYER) {
    const CFwd f = {actor, X, lo.ldsa, lo.B, w.hp};
    if ((rc = crr_forward(n, &f, 1, ws, st)) != OSA_OK) return rc;
    g.pre = ws + w.hp[top];
    hipLaunchKernelGGL(sac_head_row_kernel, dim3(crr_blocks(lo.B, 4)), dim3(256), 0, st, g);
    return OSA_OK;
  }
  for (int l = 0; l < top; ++l) {
    GArgs ga = {};
    ga.splits = 1;
    GProb p = crr_prob();
    p.A = l == 0 ? X : ws + w.hp[l - 1];
    p.lda = l == 0 ? lo.ldsa : n.ldh[l - 1];
    p.B = actor + n.oW[l]; p.ldb = n.ld[l];
    p.C = ws + w.hp[l]; p.ldc = n.ldh[l];
    p.M = lo.B; p.N = n.out[l]; p.K = n.in[l];
    p.bias = actor + n.ob[l];
    p.act = n.act;
    ga.p[ga.nprob++] = p;
    if ((rc = gm_gemm<false, false>(ga, st)) != OSA_OK) return rc;
  }
  g.H = ws + w.hp[top - 1]; g.W = actor + n.oW[top]; g.bias = actor + n.ob[top];
  hipLaunchKernelGGL(sac_head_kernel, dim3(crr_blocks(lo.B, BC_ROWS)), dim3(256), 0, st, g);
  return OSA_OK;
}

// ---- the temperature (sac.py:163-176) and the end of a step --------------------------------------------------------------
struct SAlpha {
  const float* logp;
  float* la;  // log alpha, exp_avg, exp_avg_sq
  int* t;
  float* stats;
  const long* step;
  int nslots, B;
  float lr, target;
  double beta1, beta2, eps;
};
__global__ __launch_bounds__(256) void sac_alpha_kernel(SAlpha g) {
  __shared__ double red[17];
  double s = 0.0;
  for (int b = threadIdx.x; b < g.B; b += 256) s += (double)g.logp[b];
  s = osa_block_sum<256>(s, red);
  if (threadIdx.x == 0) {
    const float mean = (float)(s / g.B) + g.target, la = g.la[0];
    const int t = *g.t + 1;
    *g.t = t;
    float m = g.la[1], v = g.la[2];
    g.la[0] = crr_adam1(-mean, m, v, la, g.lr, g.beta1, g.beta2, g.eps, t);  // d(-log_alpha mean)/dlog_alpha
    g.la[1] = m;
    g.la[2] = v;
    g.stats[(*g.step % g.nslots) * OSA_SAC_NSTAT + 6] = -la * mean;
  }
}
__global__ void sac_finish_kernel(long* step, const float* la, float* stats, int nslots, int actor_step, int alpha_step) {
  if (threadIdx.x != 0) return;
  float* s = stats + (*step % nslots) * OSA_SAC_NSTAT;
  s[5] = expf(la[0]);
  if (!actor_step) s[2] = 0.f;
  if (!alpha_step) s[6] = 0.f;
  *step += 1;
}

// ---- draws, act ----------------------------------------------------------------------------------------------------
#define SAC_KEY_IDX 0x53414349445831ull /* keys of their own: seed ^ key, counter = (step, element) */
#define SAC_KEY_EPS 0x53414345505331ull
#define SAC_KEY_ACT 0x53414341435431ull

__global__ __launch_bounds__(256) void sac_draw_kernel(unsigned long long seed, long first, int nsteps, int nslots, int B,
                                                       int A, const long* __restrict__ pos, long* __restrict__ idx,
                                                       float* __restrict__ eps) {
  const long per = (long)B * (1 + 3 * A), e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= nsteps * per) return;
  const long k = e / per, i = e - k * per, step = first + k, slot = step % nslots;
  uint32_t w[4];
  if (i < B) {
    const long fill = pos[1] > 0 ? pos[1] : 1;
    osa_philox(seed ^ SAC_KEY_IDX, (uint64_t)step, (uint64_t)i, w);
    const unsigned long long bits = (unsigned long long)w[0] | ((unsigned long long)w[1] << 32);
    idx[slot * B + i] = (long)__umul64hi(bits, (unsigned long long)fill);
  } else {
    osa_philox(seed ^ SAC_KEY_EPS, (uint64_t)step, (uint64_t)(i - B), w);
    eps[slot * (long)3 * B * A + (i - B)] = td3_normal(w);
  }
}

// one row per workgroup; a wave per output column, lanes over K, the wave's sum in a fixed order
struct SAct {
  BNetK net;
  const float *p, *obs;
  float* out;
  int D, A, ld_obs, ld_out, mode;
  unsigned long long key, offset;
};
constexpr int S_ACT_W = 4096;
__global__ __launch_bounds__(256) void sac_act_kernel(SAct g) {
  __shared__ float buf[2][S_ACT_W];
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
      if (lane == 0) buf[cur ^ 1][n] = gm_act(s + b[n], l + 1 < nk.L ? nk.act : OSA_ACT_IDENTITY);
    }
    __syncthreads();
    cur ^= 1;
    K = N;
  }
  if (tid < g.A) {
    float eps = 0.f;
    if (g.mode == 0) {  // GaussianSACActor.predict(deterministic=False)
      osa_philox(g.key, g.offset, (uint64_t)row * g.A + tid, w);
      eps = td3_normal(w);
    }
    const SHeadOut o = sac_head1(buf[cur][tid], buf[cur][g.A + tid], eps);
    g.out[(long)row * g.ld_out + tid] = g.mode == 0 ? o.a : o.tm;
  }
}

}  // namespace

extern "C" {

int osa_sac_layout(const osa_sac_desc* desc, int* out) {
  SLayout lo;
  OSA_REQUIRE(desc && out);
  const int rc = sac_make_layout(desc, &lo);
  if (rc != OSA_OK) return rc;
  out[0] = lo.pi.P; out[1] = lo.q.P; out[2] = OSA_SAC_NSTAT; out[3] = 0;
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

size_t osa_sac_ws_floats(const osa_sac_desc* desc) {
  SLayout lo;
  if (sac_make_layout(desc, &lo) != OSA_OK) return 0;
  return sac_ws(lo).total;
}

int osa_sac_head_supported(const osa_sac_desc* desc) {
  SLayout lo;
  return sac_make_layout(desc, &lo) == OSA_OK && sac_head_ok(lo) ? 1 : 0;
}

int osa_sac_draws(const osa_sac_desc* desc, unsigned long long seed, long first_step, int nsteps, int nslots,
                  const osa_td3_ring* ring, long* idx, float* eps, void* stream) {
  SLayout lo;
  OSA_REQUIRE(desc && idx && eps);
  const int rc = sac_make_layout(desc, &lo);
  if (rc != OSA_OK) return rc;
  OSA_REQUIRE(first_step >= 0 && nsteps >= 1 && nslots >= 1 && nsteps <= nslots && td3_ring_ok(ring, lo.D, lo.A));
  hipLaunchKernelGGL(sac_draw_kernel, dim3(crr_blocks((long)nsteps * lo.B * (1 + 3 * lo.A), 256)), dim3(256), 0,
                     osa_stream(stream), seed, first_step, nsteps, nslots, lo.B, lo.A, ring->pos, idx, eps);
  OSA_CHECK_LAUNCH();
  return OSA_OK;
}

int osa_sac_step(const osa_sac_desc* desc, const osa_sac_hparams* hp, const osa_sac_state* s, const osa_td3_ring* ring,
                 const osa_sac_draw_buffers* dr, float* stats, float* ws, size_t ws_floats, long update_count, int nsteps,
                 void* stream) {
  SLayout lo;
  OSA_REQUIRE(desc && hp && s && ring && dr && stats && ws && nsteps >= 1 && update_count >= 0);
  int rc = sac_make_layout(desc, &lo);
  if (rc != OSA_OK) return rc;
  OSA_REQUIRE(hp->head == OSA_SAC_HEAD_LAYER || hp->head == OSA_SAC_HEAD_FUSED);
  if (hp->head == OSA_SAC_HEAD_FUSED && !sac_head_ok(lo)) return OSA_EUNSUPPORTED;
  const SWs w = sac_ws(lo);
  OSA_REQUIRE(ws_floats >= w.total && (reinterpret_cast<uintptr_t>(ws) & 15) == 0);
  OSA_REQUIRE(s->actor && s->actor_m && s->actor_v && s->actor_t && s->critic && s->critic_m && s->critic_v &&
              s->critic_t && s->adam_step && s->step && s->log_alpha);
  OSA_REQUIRE(td3_ring_ok(ring, lo.D, lo.A) && dr->idx && dr->eps && dr->nslots >= 1);
  OSA_REQUIRE(hp->policy_delay >= 1 && hp->lr_actor >= 0.f && hp->lr_critic >= 0.f && hp->lr_alpha >= 0.f &&
              hp->max_grad_norm >= 0.f && hp->critic_norm_coeff >= 0.f && hp->beta1 >= 0.0 && hp->beta1 < 1.0 &&
              hp->beta2 >= 0.0 && hp->beta2 < 1.0 && (hp->auto_alpha == 0 || hp->auto_alpha == 1));
  for (const float* p : {s->actor, s->actor_m, s->actor_v, s->actor_t, s->critic, s->critic_m, s->critic_v, s->critic_t})
    OSA_REQUIRE((reinterpret_cast<uintptr_t>(p) & 15) == 0);
  hipStream_t st = osa_stream(stream);
  const int B = lo.B, top = lo.q.L - 1, nc = lo.nc, ptop = lo.pi.L - 1;
  const long Pc = lo.q.P;
  double* part = reinterpret_cast<double*>(ws + w.part);
  SHead hd = {};
  hd.eps = dr->eps; hd.step = s->step; hd.nslots = dr->nslots;
  for (int it = 0; it < nsteps; ++it) {
    const bool actor_step = (update_count + it + 1) % hp->policy_delay == 0;  // ddpg.py:398
    // ---- the critics: ONE forward of the online actor on next_obs feeds the reward target (a', log pi) and the cost
    // target (tanh mu, ddpg.py:471)
    TGather ga = {*ring, dr->idx, s->step, dr->nslots, B, lo.D, lo.A, lo.ldsa, ws + w.xq, ws + w.xn[0],
                  lo.cost ? ws + w.xn[1] : nullptr, ws + w.rcd};
    hipLaunchKernelGGL(td3_gather_kernel, dim3(crr_blocks(B, 4)), dim3(256), 0, st, ga);
    SHead ht = hd;
    ht.draw = 0; ht.xa = ws + w.xn[0]; ht.xb = lo.cost ? ws + w.xn[1] : nullptr; ht.logp = ws + w.logp;
    if ((rc = sac_actor_forward(lo, w, hp->head, s->actor, ws + w.xn[0], ht, ws, st)) != OSA_OK) return rc;
    CFwd tf[3], of[3];
    for (int j = 0; j < nc; ++j) {
      tf[j] = {s->critic_t + j * Pc, ws + w.xn[j >= 2 ? 1 : 0], lo.ldsa, B, w.ht[j]};
      of[j] = {s->critic + j * Pc, ws + w.xq, lo.ldsa, B, w.ho[j]};
    }
    if ((rc = crr_forward(lo.q, tf, nc, ws, st)) != OSA_OK) return rc;
    if ((rc = crr_forward(lo.q, of, nc, ws, st)) != OSA_OK) return rc;
    STd td = {};
    for (int j = 0; j < nc; ++j) {
      td.q[j] = ws + w.ho[j][top]; td.tq[j] = ws + w.ht[j][top]; td.dz[j] = ws + w.z[j][0];
    }
    td.rcd = ws + w.rcd; td.logp = ws + w.logp; td.log_alpha = s->log_alpha; td.rows = ws + w.rows;
    td.B = B; td.cost = lo.cost; td.gamma = hp->gamma;
    hipLaunchKernelGGL(sac_td_kernel, dim3(crr_blocks(B, 256)), dim3(256), 0, st, td);
    CBwd cb[3];
    for (int j = 0; j < nc; ++j)
      cb[j] = {s->critic + j * Pc, ws + w.xq, lo.ldsa, w.ho[j], {w.z[j][0], w.z[j][1]}, ws + w.gq + j * Pc};
    if ((rc = crr_backward(lo.q, cb, nc, B, ws, st)) != OSA_OK) return rc;
    TNorm nr = {{ws + w.gq, ws + w.gq + 2 * Pc}, {s->critic, s->critic + 2 * Pc}, {2 * Pc, Pc},
                {s->adam_step + 1, s->adam_step + 2}, part, hp->critic_norm_coeff};
    hipLaunchKernelGGL(td3_norm_kernel, dim3(T_NB, 1 + lo.cost), dim3(256), 0, st, nr);
    TAdam ad = {lo.q.Pn, 2, B, dr->nslots, 0, Pc, (long)w.hstride, s->critic, s->critic_m, s->critic_v,
                actor_step ? s->critic_t : nullptr, stats, ws + w.gq, ws + w.rows, ws + w.ho[0][top], part,
                s->adam_step + 1, s->step, hp->lr_critic, hp->max_grad_norm, hp->critic_norm_coeff, hp->polyak,
                hp->one_minus_polyak, hp->beta1, hp->beta2, hp->adam_eps};
    hipLaunchKernelGGL(td3_adam_kernel, dim3(crr_blocks(lo.q.Pn, 256), nc), dim3(256), 0, st, ad);
    if (actor_step) {  // sac.py:178-207 with the UPDATED critics
      SHead ha = hd;
      ha.draw = 1; ha.xsrc = ws + w.xq; ha.xa = ws + w.xc; ha.logp = ws + w.logp;
      ha.sa = ws + w.sa; ha.sse = ws + w.sse; ha.smask = ws + w.smask;
      if ((rc = sac_actor_forward(lo, w, hp->head, s->actor, ws + w.xq, ha, ws, st)) != OSA_OK) return rc;
      const CFwd qf[2] = {{s->critic, ws + w.xc, lo.ldsa, B, w.hq[0]}, {s->critic + Pc, ws + w.xc, lo.ldsa, B, w.hq[1]}};
      if ((rc = crr_forward(lo.q, qf, 2, ws, st)) != OSA_OK) return rc;
      hipLaunchKernelGGL(sac_dq_kernel, dim3(crr_blocks(B, 256)), dim3(256), 0, st, B, ws + w.hq[0][top],
                         ws + w.hq[1][top], ws + w.logp, s->log_alpha, ws + w.z[0][0], ws + w.z[1][0], ws + w.nl);
      if ((rc = sac_critics_dx(lo.q, s->critic, w, B, lo.ldsa, ws, st)) != OSA_OK) return rc;
      SGrad sg = {};
      sg.dx0 = ws + w.dx[0]; sg.dx1 = ws + w.dx[1]; sg.sa = ws + w.sa; sg.sse = ws + w.sse; sg.smask = ws + w.smask;
      sg.log_alpha = s->log_alpha;
      sg.B = B; sg.A = lo.A; sg.D = lo.D; sg.K = lo.K; sg.ldk = lo.ldk; sg.ld2 = lo.ld2; sg.ldsa = lo.ldsa;
      sg.lda = lo.lda; sg.act = lo.pi.act;
      CBwd pb = {s->actor, ws + w.xq, lo.ldsa, w.hp, {w.z[2][0], w.z[2][1]}, ws + w.gp};
      if (hp->head == OSA_SAC_HEAD_LAYER) {
        sg.dz = ws + w.z[2][0];
        hipLaunchKernelGGL(sac_dhead_row_kernel, dim3(crr_blocks((long)B * lo.ld2, 256)), dim3(256), 0, st, sg);
        if ((rc = crr_backward(lo.pi, &pb, 1, B, ws, st)) != OSA_OK) return rc;
      } else {  // the top layer's dW, db and the dZ of the last hidden layer in one launch; the layers below as ever
        sg.H = ws + w.hp[ptop - 1]; sg.W = s->actor + lo.pi.oW[ptop];
        sg.gW = ws + w.gp + lo.pi.oW[ptop]; sg.gb = ws + w.gp + lo.pi.ob[ptop]; sg.dH = ws + w.z[2][0];
        hipLaunchKernelGGL(sac_head_grad_kernel, dim3(crr_blocks(lo.ldk, SG_SLAB)), dim3(256), 0, st, sg);
        CNet body = lo.pi;
        body.L = ptop;
        if ((rc = crr_backward(body, &pb, 1, B, ws, st)) != OSA_OK) return rc;
      }
      double* apart = part + (long)2 * T_NB * 2;
      // (over the Pn floats the backward writes on either head route, not the block's padding up to P)
      TNorm na = {{ws + w.gp, nullptr}, {s->actor, nullptr}, {lo.pi.Pn, 0}, {s->adam_step, nullptr}, apart, 0.f};
      hipLaunchKernelGGL(td3_norm_kernel, dim3(T_NB, 1), dim3(256), 0, st, na);
      TAdam aa = {lo.pi.Pn, 1, B, dr->nslots, 1, (long)lo.pi.P, 0, s->actor, s->actor_m, s->actor_v, s->actor_t, stats,
                  ws + w.gp, nullptr, ws + w.nl, apart, s->adam_step, s->step, hp->lr_actor, hp->max_grad_norm, 0.f,
                  hp->polyak, hp->one_minus_polyak, hp->beta1, hp->beta2, hp->adam_eps};
      hipLaunchKernelGGL(td3_adam_kernel, dim3(crr_blocks(lo.pi.Pn, 256), 1), dim3(256), 0, st, aa);
      if (hp->auto_alpha) {  // sac.py:163-176: the UPDATED actor, a fresh draw
        SHead hl = hd;
        hl.draw = 2; hl.logp = ws + w.logp;
        if ((rc = sac_actor_forward(lo, w, hp->head, s->actor, ws + w.xq, hl, ws, st)) != OSA_OK) return rc;
        SAlpha al = {ws + w.logp, s->log_alpha, s->adam_step + 3, stats, s->step, dr->nslots, B, hp->lr_alpha,
                     hp->target_entropy, hp->beta1, hp->beta2, hp->adam_eps};
        hipLaunchKernelGGL(sac_alpha_kernel, dim3(1), dim3(256), 0, st, al);
      }
    }
    hipLaunchKernelGGL(sac_finish_kernel, dim3(1), dim3(64), 0, st, s->step, s->log_alpha, stats, dr->nslots,
                       (int)actor_step, (int)(actor_step && hp->auto_alpha));
    OSA_CHECK_LAUNCH();
  }
  return OSA_OK;
}

int osa_sac_act(const osa_sac_desc* desc, const float* actor, const float* obs, int ld_obs, long n, int mode,
                unsigned long long seed, unsigned long long offset, float* out, int ld_out, void* stream) {
  SLayout lo;
  OSA_REQUIRE(desc && out && n >= 1 && n <= 1024 && mode >= 0 && mode <= 2);
  const int rc = sac_make_layout(desc, &lo);
  if (rc != OSA_OK) return rc;
  OSA_REQUIRE(ld_out >= lo.A && (mode == 1 || (actor && obs && ld_obs >= lo.D)));
  SAct g = {bcq_netk(lo.pi), actor, obs, out, lo.D, lo.A, ld_obs, ld_out, mode, seed ^ SAC_KEY_ACT, offset};
  hipLaunchKernelGGL(sac_act_kernel, dim3((unsigned)n), dim3(256), 0, osa_stream(stream), g);
  OSA_CHECK_LAUNCH();
  return OSA_OK;
}

}  // extern "C"
