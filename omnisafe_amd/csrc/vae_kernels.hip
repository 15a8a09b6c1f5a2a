// Offline VAE-BC trained on the device from a device-resident dataset: the conditional VAE of
// omnisafe/models/actor/vae_actor.py:43-138, its loss and the Adam step of omnisafe/algorithms/offline/vae_bc.py:79-97,
// and VAE.decode for the players.
//
// The YAML shape is batch 256 on hidden 750 x 750: one dependent chain of layers whose outputs are 256 x 750.  On the
// 64 x 64 tiles of gm_gemm_kernel that is 48 workgroups on a 256-CU part, each wave walking the whole K range.  The
// skinny-batch kernel below (vae_skinny_kernel) gives every 32 x 32 MFMA output tile a workgroup of its own and splits
// the tile's K range over the workgroup's four waves:
//   * a wave owns one float32 32x32x2 MFMA accumulator (16 registers) and a quarter of K, rounded to whole 32-wide
//     chunks; it stages its own 32 x 32 chunk of either operand through a wave-private LDS panel ([row][k], leading
//     dimension 36: one 16-byte LDS read per fragment feeds four MFMAs) with the next chunk's global loads in flight;
//   * the four partial tiles meet in LDS and are added in wave order 0, 1, 2, 3 -- a fixed order, no atomics, no slab
//     in global memory and no second launch; every wave then finishes a quarter of the tile's rows (bias, activation,
//     activation', the bias-gradient column, zero padding);
//   * a launch takes two problems: a layer's weight gradient and the data gradient of the layer below read the same
//     dZ and leave together.
// At 256 x 750 x 750 a forward layer is 8 x 24 = 192 workgroups (768 waves, 94 MFMAs each instead of 375), a backward
// layer 24 x 24 + 8 x 24 = 768; the count is bounded by the 32 x 32 MFMA tile -- M / 32 x N / 32 -- not by K.
// Operand rows may come straight from the dataset through idx[b], and an operand's columns may continue in a second
// array (obs || act, obs || z): the first layers need no gather launch and no concatenated copy.
//
// Around it: the encoder head (chunk, clamp, exp, z, KL), the decoder head (MSE, dL/dpred), the head backward (KL
// gradient, clamp mask), one Adam launch over both networks (which also advances the device step counter), the draws.
// OSA_VAE_ROUTE_TILE runs the body layers (every layer but a network's first) on gm_gemm_kernel instead.
#include <math.h>

#include "gm_gemm.h"

namespace {

struct VNet {
  int L, in[GM_MAXL], out[GM_MAXL], ld[GM_MAXL], ldh[GM_MAXL], oW[GM_MAXL], ob[GM_MAXL];
  int Pn, P, maxldh;
};
struct VLayout {
  VNet e, d;
  int D, A, A2, B, act, lda, ld2a, ld4a;
};

inline int v4(int x) { return (x + 3) / 4 * 4; }

int vae_make_net(VNet& n, int in_dim, int nh, const int* hidden, int out_dim) {
  n.L = nh + 1;
  n.maxldh = 4;
  int off = 0, prev = in_dim;
  for (int l = 0; l < n.L; ++l) {
    const int w = l < nh ? hidden[l] : out_dim;
    if (w < 1 || w > 4096) return OSA_EINVAL;
    n.in[l] = prev; n.out[l] = w; n.ld[l] = v4(prev); n.ldh[l] = v4(w);
    if (n.ldh[l] > n.maxldh) n.maxldh = n.ldh[l];
    n.oW[l] = off; off += w * n.ld[l];
    n.ob[l] = off; off += v4(w);
    prev = w;
  }
  n.Pn = off;
  n.P = (off + 15) / 16 * 16;
  return OSA_OK;
}

int vae_make_layout(const osa_vae_desc* d, VLayout* lo) {
  if (!d) return OSA_EINVAL;
  if (d->obs_dim < 1 || d->obs_dim > 4096 || d->act_dim < 1 || d->batch < 1) return OSA_EINVAL;
  if (d->n_hidden < 1 || d->n_hidden + 1 > GM_MAXL || d->act_dim > 32 || d->batch > (1 << 20)) return OSA_EUNSUPPORTED;
  if (d->activation < OSA_ACT_TANH || d->activation > OSA_ACT_IDENTITY) return OSA_EUNSUPPORTED;
  lo->D = d->obs_dim; lo->A = d->act_dim; lo->A2 = 2 * d->act_dim; lo->B = d->batch; lo->act = d->activation;
  lo->lda = v4(lo->A); lo->ld2a = v4(lo->A2); lo->ld4a = v4(2 * lo->A2);
  const int rc = vae_make_net(lo->e, lo->D + lo->A, d->n_hidden, d->hidden, 2 * lo->A2);
  if (rc != OSA_OK) return rc;
  return vae_make_net(lo->d, lo->D + lo->A2, d->n_hidden, d->hidden, lo->A);
}

bool vae_skinny_ok(const VLayout& lo) { return lo.B <= 512; }

struct VWs {
  size_t he[GM_MAXL], hd[GM_MAXL], z, sig, msk, dz[2], dzl, grad, red, total;
};
VWs vae_ws(const VLayout& lo) {
  VWs w;
  size_t off = 0;
  auto take = [&](size_t n) {
    const size_t o = off;
    off += (n + 3) / 4 * 4;
    return o;
  };
  const size_t B = lo.B;
  for (int l = 0; l < GM_MAXL; ++l) w.he[l] = l < lo.e.L ? take(B * lo.e.ldh[l]) : 0;
  for (int l = 0; l < GM_MAXL; ++l) w.hd[l] = l < lo.d.L ? take(B * lo.d.ldh[l]) : 0;
  w.z = take(B * lo.ld2a);
  w.sig = take(B * lo.ld2a);
  w.msk = take(B * lo.ld2a);
  const int mz = lo.e.maxldh > lo.d.maxldh ? lo.e.maxldh : lo.d.maxldh;
  for (int k = 0; k < 2; ++k) w.dz[k] = take(B * mz);
  w.dzl = take(B * lo.ld2a);
  w.grad = take((size_t)lo.e.P + lo.d.P);
  w.red = take(8);  // [0]: the KL loss, from the encoder head to the decoder head's statistics row
  w.total = off;
  return w;
}

// ---- the skinny-batch layer kernel -------------------------------------------------------------------------------
// An operand as it lies in memory: rows of `ld` floats.  idx: memory row r is row idx[slot][r] of the dataset.  p2: the
// columns from `split` on continue in p2[r][c - split] (idx2: gathered like p, else plain rows).  vec: 16-byte loads are
// safe (no idx, no p2, aligned base, ld a multiple of 4).
struct SSrc {
  const float* p;
  const float* p2;
  int ld, ld2, split, idx, idx2, vec;
};
// C[m][n] = epi(sum_k A(m, k) B(k, n)).  at: A(m, k) = A[k][m] (else A[m][k]); bt: B(k, n) = B[k][n] (else B[n][k]).
// The epilogue is gm_gemm_kernel's: + bias[n], activation, * act'(aux[m][n]); ones_n >= 0 (with bt): B(k, ones_n) = 1,
// that column of the product goes to cb[m] (the bias gradient), cb[M .. cb_pad) and C[m][N .. ldc) are written zero.
struct SProb {
  SSrc A, Bm;
  float* C;
  const float* bias;
  const float* aux;
  float* cb;
  int at, bt, M, N, K, ldc, ldaux, act, dact, ones_n, cb_pad;
};
struct SArgs {
  SProb p[2];
  int nprob;
  const long* idx;   // [nslots][B]
  const long* step;
  int nslots, B;
  long nrows;        // rows of the dataset
};

constexpr int SK_T = 32;        // tile edge = the MFMA's, and the K chunk of a stage
constexpr int SK_LD = SK_T + 4; // leading dimension of an LDS panel

// four floats of memory row mr from column mc on, zero where !ok or the column is >= lim
__device__ __forceinline__ f32x4 sk_fetch(const SSrc& s, const long* __restrict__ idx, long nrows, int mr, int mc, int lim,
                                          bool ok) {
  if (s.vec) return gm_load4(s.p + (long)mr * s.ld, mc, lim, ok);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (!ok || mc >= lim) return v;
  long g = mr;
  if (s.idx) {
    g = idx[mr];
    if (g < 0 || g >= nrows) g = 0;  // (injected indices are checked on the host; never read outside the dataset)
  }
  const float* r1 = s.p + g * s.ld;
  const float* r2 = s.p2 ? s.p2 + (s.idx2 ? g : (long)mr) * s.ld2 - s.split : nullptr;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = mc + i;
    if (c < lim) v[i] = (r2 && c >= s.split) ? r2[c] : r1[c];
  }
  return v;
}

__global__ __launch_bounds__(256) void vae_skinny_kernel(SArgs g) {
  // [wave][A panel | B panel]; after the K loop the first 4 x 16 x 64 floats hold the four partial tiles
  __shared__ __attribute__((aligned(16))) float smem[4 * 2 * SK_T * SK_LD];
  const SProb p = blockIdx.z == 0 ? g.p[0] : g.p[1];
  const int M = p.M, N = p.N, K = p.K;
  const int ncols = p.ones_n >= 0 ? (p.ldc > N + 1 ? p.ldc : N + 1) : N;
  const int m0 = blockIdx.y * SK_T, n0 = blockIdx.x * SK_T;
  if (m0 >= M || n0 >= ncols) return;  // (the grid follows the launch's largest problem)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, kk = lane >> 5;
  const long* __restrict__ idx = g.idx ? g.idx + (*g.step % g.nslots) * g.B : nullptr;  // (null: no gathered operand)
  // this wave's quarter of K in whole chunks; every wave runs the same number of stages (the barriers are uniform)
  const int nst = (K + 4 * SK_T - 1) / (4 * SK_T);
  const int kbeg = wave * nst * SK_T;
  const int kend = K < kbeg + nst * SK_T ? K : kbeg + nst * SK_T;
  float* sA = smem + wave * 2 * SK_T * SK_LD;
  float* sB = sA + SK_T * SK_LD;
  f32x4 ra[4], rb[4];
  auto load_chunk = [&](int s) {
    const int k0 = kbeg + s * SK_T;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int u = lane + 64 * q, hi = u >> 3, c = 4 * (u & 7);
      // at: memory row = k, 32 consecutive m; else memory row = m, 32 consecutive k
      ra[q] = p.at ? sk_fetch(p.A, idx, g.nrows, k0 + hi, m0 + c, M, k0 + hi < kend)
                   : sk_fetch(p.A, idx, g.nrows, m0 + hi, k0 + c, kend, m0 + hi < M);
      if (p.bt) {
        f32x4 v = sk_fetch(p.Bm, idx, g.nrows, k0 + hi, n0 + c, N, k0 + hi < kend);
        if (p.ones_n >= 0 && k0 + hi < kend) {  // the column of ones: the bias gradient is one more output column
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (n0 + c + i == p.ones_n) v[i] = 1.f;
        }
        rb[q] = v;
      } else {
        rb[q] = sk_fetch(p.Bm, idx, g.nrows, n0 + hi, k0 + c, kend, n0 + hi < N);
      }
    }
  };
  auto store_chunk = [&]() {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int u = lane + 64 * q, hi = u >> 3, c = 4 * (u & 7);
      if (p.at) {
#pragma unroll
        for (int i = 0; i < 4; ++i) sA[(c + i) * SK_LD + hi] = ra[q][i];
      } else {
        *reinterpret_cast<f32x4*>(&sA[hi * SK_LD + c]) = ra[q];
      }
      if (p.bt) {
#pragma unroll
        for (int i = 0; i < 4; ++i) sB[(c + i) * SK_LD + hi] = rb[q][i];
      } else {
        *reinterpret_cast<f32x4*>(&sB[hi * SK_LD + c]) = rb[q];
      }
    }
  };
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  if (kbeg < kend) load_chunk(0);
  for (int s = 0; s < nst; ++s) {
    const bool live = kbeg + s * SK_T < kend;  // wave-uniform
    __syncthreads();                            // the panels' last readers are done
    if (live) store_chunk();
    __syncthreads();
    if (kbeg + (s + 1) * SK_T < kend && s + 1 < nst) load_chunk(s + 1);  // in flight under this chunk's MFMAs
    if (live) {
#pragma unroll
      for (int j = 0; j < SK_T / 8; ++j) {
        // lane group kk consumes k = 8 j + 4 kk + q in MFMA step q, for A and B alike
        const f32x4 af = *reinterpret_cast<const f32x4*>(&sA[l31 * SK_LD + 8 * j + 4 * kk]);
        const f32x4 bf = *reinterpret_cast<const f32x4*>(&sB[l31 * SK_LD + 8 * j + 4 * kk]);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[q], bf[q], acc, 0, 0, 0);
      }
    }
  }
  // ---- the ordered reduce: partial tile of wave w at smem[w][r][lane]
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 16; ++r) smem[(wave * 16 + r) * 64 + lane] = acc[r];
  __syncthreads();
  const int n = n0 + l31;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = 4 * wave + i;
    float v = smem[(0 * 16 + r) * 64 + lane];
    v += smem[(1 * 16 + r) * 64 + lane];
    v += smem[(2 * 16 + r) * 64 + lane];
    v += smem[(3 * 16 + r) * 64 + lane];
    const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * kk;  // D[row][col = l31] of the 32 x 32 MFMA
    if (m < M) {
      if (n < N) {
        if (p.bias) v += p.bias[n];
        if (p.act >= 0) v = gm_act(v, p.act);
        if (p.dact >= 0) v *= gm_dact(p.aux[(long)m * p.ldaux + n], p.dact);
        p.C[(long)m * p.ldc + n] = v;
      } else {
        if (n == p.ones_n && p.cb) p.cb[m] = v;
        if (n < p.ldc && p.ones_n >= 0) p.C[(long)m * p.ldc + n] = 0.f;  // padding columns of the weight block
      }
    } else if (n == p.ones_n && p.cb && m < p.cb_pad) {
      p.cb[m] = 0.f;  // padding of the bias block
    }
  }
}

SSrc sk_plain(const float* p, int ld) {
  SSrc s = {};
  s.p = p;
  s.ld = ld;
  s.split = 1 << 30;
  s.vec = (reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % 4 == 0;
  return s;
}
// dataset rows through idx (gather != 0) or plain rows, continued from column `split` in p2
SSrc sk_concat(const float* p, int ld, int gather, int split, const float* p2, int ld2, int gather2) {
  SSrc s = {};
  s.p = p; s.ld = ld; s.idx = gather; s.split = split; s.p2 = p2; s.ld2 = ld2; s.idx2 = gather2;
  return s;
}
SProb sk_prob() {
  SProb p = {};
  p.act = -1;
  p.dact = -1;
  p.ones_n = -1;
  return p;
}

struct VCtx {  // what every launch of a step shares
  const long* idx;
  const long* step;
  int nslots, B;
  long nrows;
  bool tile;  // body layers on gm_gemm_kernel
  hipStream_t st;
};

int sk_launch(const VCtx& c, const SProb* p, int n) {
  SArgs g = {};
  int tx = 0, ty = 0;
  for (int i = 0; i < n; ++i) {
    g.p[i] = p[i];
    const int nc = p[i].ones_n >= 0 ? (p[i].ldc > p[i].N + 1 ? p[i].ldc : p[i].N + 1) : p[i].N;
    if ((nc + SK_T - 1) / SK_T > tx) tx = (nc + SK_T - 1) / SK_T;
    if ((p[i].M + SK_T - 1) / SK_T > ty) ty = (p[i].M + SK_T - 1) / SK_T;
  }
  if (tx == 0 || ty == 0) return OSA_OK;
  if (ty > 65535) return OSA_EUNSUPPORTED;
  g.nprob = n; g.idx = c.idx; g.step = c.step; g.nslots = c.nslots; g.B = c.B; g.nrows = c.nrows;
  hipLaunchKernelGGL(vae_skinny_kernel, dim3(tx, ty, n), dim3(256), 0, c.st, g);
  return hipGetLastError() == hipSuccess ? OSA_OK : OSA_EHIP;
}

// a body layer's problems: together on the skinny kernel, or one launch each on the tile GEMM
int vae_body(const VCtx& c, const SProb* p, int n) {
  if (!c.tile) return sk_launch(c, p, n);
  for (int i = 0; i < n; ++i) {
    GArgs g = {};
    g.splits = 1;
    g.nprob = 1;
    GProb& q = g.p[0];
    q.A = p[i].A.p; q.lda = p[i].A.ld; q.B = p[i].Bm.p; q.ldb = p[i].Bm.ld; q.C = p[i].C; q.ldc = p[i].ldc;
    q.bias = p[i].bias; q.aux = p[i].aux; q.ldaux = p[i].ldaux; q.cb = p[i].cb; q.cb_pad = p[i].cb_pad;
    q.M = p[i].M; q.N = p[i].N; q.K = p[i].K; q.act = p[i].act; q.dact = p[i].dact; q.ones_n = p[i].ones_n;
    q.splits = 1;
    const int rc = p[i].at ? gm_gemm<true, true>(g, c.st)
                           : (p[i].bt ? gm_gemm<false, true>(g, c.st) : gm_gemm<false, false>(g, c.st));
    if (rc != OSA_OK) return rc;
  }
  return OSA_OK;
}

// forward of one network over M rows: layer 0 reads `x0` (gathered / concatenated), layer l > 0 the output of l - 1
int vae_forward(const VCtx& c, const VNet& n, int act, const float* params, const SSrc& x0, int M, float* const* h,
                const int* ldh) {
  for (int l = 0; l < n.L; ++l) {
    SProb p = sk_prob();
    p.A = l == 0 ? x0 : sk_plain(h[l - 1], ldh[l - 1]);
    p.Bm = sk_plain(params + n.oW[l], n.ld[l]);
    p.C = h[l]; p.ldc = ldh[l];
    p.M = M; p.N = n.out[l]; p.K = n.in[l];
    p.bias = params + n.ob[l];
    p.act = l + 1 < n.L ? act : -1;
    const int rc = l == 0 ? sk_launch(c, &p, 1) : vae_body(c, &p, 1);
    if (rc != OSA_OK) return rc;
  }
  return OSA_OK;
}

// backward of one network over B rows.  dz[0] holds dL/d(top pre-activation) on entry.  Per layer: dW_l (+ db_l)
// straight into the gradient block and dZ of the layer below, one launch for both on the skinny route.  latent != null:
// the first layer's data gradient for the columns lat0 .. lat0 + latn of its input alone.
int vae_backward(const VCtx& c, const VNet& n, int act, const float* params, const SSrc& x0, float* const* h,
                 float* const dz[2], float* grad, float* latent, int lat0, int latn, int ldlat) {
  int cur = 0;
  for (int l = n.L - 1; l >= 0; --l) {
    SProb p[2];
    p[0] = sk_prob();  // dW_l[out][in] (+ db_l) = dZ_l^T [out][rows] . {H_{l-1}, 1}[rows][in + 1]
    p[0].at = 1; p[0].bt = 1;
    p[0].A = sk_plain(dz[cur], n.ldh[l]);
    p[0].Bm = l == 0 ? x0 : sk_plain(h[l - 1], n.ldh[l - 1]);
    p[0].C = grad + n.oW[l]; p[0].ldc = n.ld[l];
    p[0].cb = grad + n.ob[l]; p[0].cb_pad = v4(n.out[l]);
    p[0].M = n.out[l]; p[0].N = n.in[l]; p[0].K = c.B;
    p[0].ones_n = n.in[l];
    int np = 1;
    if (l > 0 || latent) {  // dZ_{l-1}[rows][in] = (dZ_l[rows][out] . W_l[out][in]) * act'(H_{l-1})
      SProb& q = p[1];
      q = sk_prob();
      q.bt = 1;
      q.A = sk_plain(dz[cur], n.ldh[l]);
      q.M = c.B; q.K = n.out[l];
      if (l > 0) {
        q.Bm = sk_plain(params + n.oW[l], n.ld[l]);
        q.C = dz[cur ^ 1]; q.ldc = n.ldh[l - 1]; q.N = n.in[l];
        q.dact = act; q.aux = h[l - 1]; q.ldaux = n.ldh[l - 1];
      } else {
        q.Bm = sk_plain(params + n.oW[0] + lat0, n.ld[0]);
        q.C = latent; q.ldc = ldlat; q.N = latn;
      }
      np = 2;
    }
    const int rc = l == 0 ? sk_launch(c, p, np) : vae_body(c, p, np);
    if (rc != OSA_OK) return rc;
    cur ^= 1;
  }
  return OSA_OK;
}

// ---- draws -------------------------------------------------------------------------------------------------------
#define VAE_KEY_IDX 0x56414549445831ull /* keys of their own: seed ^ key, counter = (step, element) */
#define VAE_KEY_EPS 0x56414545505331ull

// idx[slot][b]: 64 random bits, multiply-high into [0, N)
__global__ __launch_bounds__(256) void vae_draw_idx_kernel(unsigned long long seed, long first, int nsteps, int nslots,
                                                           int B, unsigned long long N, long* __restrict__ idx) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)nsteps * B) return;
  const long k = e / B, b = e - k * B, step = first + k;
  uint32_t w[4];
  osa_philox(seed ^ VAE_KEY_IDX, (uint64_t)step, (uint64_t)b, w);
  const unsigned long long bits = (unsigned long long)w[0] | ((unsigned long long)w[1] << 32);
  idx[(step % nslots) * B + b] = (long)__umul64hi(bits, N);
}
// the first Box-Muller normal of the Philox words, evaluated in double and rounded once: a host restatement in float64
// gives the same float32 whatever the last bits of either side's log and cos
__device__ __forceinline__ float vae_normal(const uint32_t* w) {
  const double u1 = (double)osa_u01(w[0]), u2 = (double)osa_u01(w[1]);
  return (float)(sqrt(-2.0 * log(u1)) * cos(6.28318530717958647692 * u2));
}
// eps[slot][i]: Philox(key, step, i)
__global__ __launch_bounds__(256) void vae_draw_eps_kernel(unsigned long long key, long first, int nsteps, int nslots,
                                                           long per_step, float* __restrict__ eps) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)nsteps * per_step) return;
  const long k = e / per_step, i = e - k * per_step, step = first + k;
  uint32_t w[4];
  osa_philox(key, (uint64_t)step, (uint64_t)i, w);
  eps[(step % nslots) * per_step + i] = vae_normal(w);
}
// the players' latent: z[r][d] = the normal of Philox(seed, offset, r A2 + d); the row's padding is written zero
__global__ __launch_bounds__(256) void vae_draw_z_kernel(unsigned long long seed, unsigned long long offset, long n,
                                                         int A2, int ldz, float* __restrict__ z) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n * ldz) return;
  const long r = e / ldz;
  const int d = (int)(e - r * ldz);
  float v = 0.f;
  if (d < A2) {
    uint32_t w[4];
    osa_philox(seed, offset, (uint64_t)(r * A2 + d), w);
    v = vae_normal(w);
  }
  z[e] = v;
}

// ---- heads -------------------------------------------------------------------------------------------------------
struct VHead {
  const float* he;   // [B][ld4a]: mu | log_std as the encoder's last layer leaves them
  const float* eps;  // [nslots][B][A2]
  const long* step;
  float *z, *sig, *msk;  // [B][ld2a]: the latent, sigma, 1 where the clamp let log_std through
  float* red;
  int nslots, B, A2, ld2a, ld4a;
};
// vae_actor.py:78-81, 108, 111: chunk, clamp, exp, rsample and the KL against N(0, 1) (torch's kl_normal_normal)
__global__ __launch_bounds__(256) void vae_enc_head_kernel(VHead g) {
  __shared__ double red[17];
  const float* eps = g.eps + (*g.step % g.nslots) * (long)g.B * g.A2;
  double kl = 0.0;
  for (int e = threadIdx.x; e < g.B * g.A2; e += 256) {
    const int b = e / g.A2, j = e - b * g.A2;
    const float mu = g.he[(long)b * g.ld4a + j], raw = g.he[(long)b * g.ld4a + g.A2 + j];
    const float ls = fminf(fmaxf(raw, -20.f), 2.f);
    const float sg = expf(ls), var = sg * sg;
    const long o = (long)b * g.ld2a + j;
    g.z[o] = __fadd_rn(mu, __fmul_rn(eps[e], sg));  // Normal.rsample: loc + eps * scale
    g.sig[o] = sg;
    g.msk[o] = (raw >= -20.f && raw <= 2.f) ? 1.f : 0.f;  // torch.clamp's backward
    kl += (double)(0.5f * (var + mu * mu - 1.f - logf(var)));
  }
  kl = osa_block_sum<256>(kl, red);
  if (threadIdx.x == 0) g.red[0] = (float)(kl / ((double)g.B * g.A2));
}

struct VLoss {
  const float* pred;  // [B][lda]
  const float* act;   // dataset actions
  const long* idx;
  const long* step;
  const float* red;
  float* dz;          // [B][lda]
  float* stats;
  int* adam_step;
  int nslots, B, A, lda, ld_act;
  long nrows;
};
// vae_actor.py:110 and vae_bc.py:85-97: the MSE against the dataset's action, dL/dpred, the step's statistics row
__global__ __launch_bounds__(256) void vae_dec_head_kernel(VLoss g) {
  __shared__ double red[17];
  const long slot = *g.step % g.nslots;
  const long* idx = g.idx + slot * g.B;
  const float scale = 2.f / (float)(g.B * g.A);
  double se = 0.0;
  for (int e = threadIdx.x; e < g.B * g.lda; e += 256) {
    const int b = e / g.lda, a = e - b * g.lda;
    float d = 0.f;
    if (a < g.A) {
      long i = idx[b];
      if (i < 0 || i >= g.nrows) i = 0;
      const float diff = g.pred[e] - g.act[i * g.ld_act + a];
      se += (double)diff * diff;
      d = diff * scale;
    }
    g.dz[e] = d;
  }
  se = osa_block_sum<256>(se, red);
  if (threadIdx.x == 0) {
    float* s = g.stats + slot * OSA_VAE_NSTAT;
    const float recon = (float)(se / ((double)g.B * g.A)), kl = g.red[0];
    s[0] = recon + kl;
    s[1] = recon;
    s[2] = kl;
    s[3] = 0.f;
    *g.adam_step += 1;
  }
}

struct VHeadBwd {
  const float *he, *eps, *sig, *msk, *dzl;  // dzl [B][ld2a]: dL_recon/dz
  const long* step;
  float* dz;                                // [B][ld4a]: dL/d(encoder output)
  int nslots, B, A2, ld2a, ld4a;
};
// through rsample, exp and clamp, with the KL's gradient folded in: dKL/dmu = mu / n, dKL/dlog_std = (sigma^2 - 1) / n
__global__ __launch_bounds__(256) void vae_head_bwd_kernel(VHeadBwd g) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)g.B * g.ld4a) return;
  const int b = (int)(e / g.ld4a), c = (int)(e - (long)b * g.ld4a);
  const float inv = 1.f / (float)(g.B * g.A2);
  float d = 0.f;
  if (c < g.A2) {
    d = g.dzl[(long)b * g.ld2a + c] + g.he[e] * inv;
  } else if (c < 2 * g.A2) {
    const int j = c - g.A2;
    const long o = (long)b * g.ld2a + j;
    const float sg = g.sig[o];
    const float ep = g.eps[((*g.step % g.nslots) * (long)g.B + b) * g.A2 + j];
    d = (g.dzl[o] * ep * sg + (sg * sg - 1.f) * inv) * g.msk[o];
  }
  g.dz[e] = d;
}

// ---- Adam --------------------------------------------------------------------------------------------------------
// torch.optim.Adam's step over the joint block: the factors 1 - beta are the float32 roundings of the DOUBLE
// differences, as torch forms them, the bias corrections are taken in double; IEEE sqrt and division.  The step's last
// launch: nothing after it reads the step's slot, so its first thread advances the device step counter.
__global__ __launch_bounds__(256) void vae_adam_kernel(long P, float* __restrict__ params, float* __restrict__ m,
                                                       float* __restrict__ v, const float* __restrict__ grad,
                                                       const int* __restrict__ adam_step, long* step, float lr,
                                                       double beta1, double beta2, double eps) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e == 0) *step += 1;
  if (e >= P) return;
  const int t = *adam_step;
  const float b2 = (float)beta2, omb1 = (float)(1.0 - beta1), omb2 = (float)(1.0 - beta2);
  const float gr = grad[e];
  const float mm = fmaf(gr - m[e], omb1, m[e]);  // exp_avg.lerp_(grad, 1 - beta1)
  const float vv = fmaf(gr * gr, omb2, v[e] * b2);
  const float step_size = (float)((double)lr / (1.0 - pow(beta1, (double)t)));
  const float bc2_sqrt = (float)sqrt(1.0 - pow(beta2, (double)t));
  const float denom = sqrtf(vv) / bc2_sqrt + (float)eps;
  params[e] = params[e] - step_size * (mm / denom);
  m[e] = mm;
  v[e] = vv;
}

unsigned vae_blocks(long n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

extern "C" {

int osa_vae_layout(const osa_vae_desc* desc, int* out) {
  VLayout lo;
  OSA_REQUIRE(desc && out);
  const int rc = vae_make_layout(desc, &lo);
  if (rc != OSA_OK) return rc;
  out[0] = lo.e.P; out[1] = lo.d.P; out[2] = OSA_VAE_NSTAT; out[3] = 0;
  int k = 4;
  for (int net = 0; net < 2; ++net) {
    const VNet& n = net == 0 ? lo.e : lo.d;
    for (int l = 0; l < OSA_GMLP_MAX_LAYERS; ++l) {
      out[k++] = l < n.L ? n.oW[l] : -1;
      out[k++] = l < n.L ? n.ob[l] : -1;
      out[k++] = l < n.L ? n.ld[l] : 0;
    }
  }
  return OSA_OK;
}

size_t osa_vae_ws_floats(const osa_vae_desc* desc) {
  VLayout lo;
  if (vae_make_layout(desc, &lo) != OSA_OK) return 0;
  return vae_ws(lo).total;
}

int osa_vae_skinny_supported(const osa_vae_desc* desc) {
  VLayout lo;
  return vae_make_layout(desc, &lo) == OSA_OK && vae_skinny_ok(lo) ? 1 : 0;
}

int osa_vae_draws(const osa_vae_desc* desc, unsigned long long seed, long first_step, int nsteps, int nslots,
                  long n_rows, long* idx, float* eps, void* stream) {
  VLayout lo;
  OSA_REQUIRE(desc && idx && eps);
  const int rc = vae_make_layout(desc, &lo);
  if (rc != OSA_OK) return rc;
  OSA_REQUIRE(first_step >= 0 && nsteps >= 1 && nslots >= 1 && nsteps <= nslots && n_rows >= 1);
  hipStream_t st = osa_stream(stream);
  hipLaunchKernelGGL(vae_draw_idx_kernel, dim3(vae_blocks((long)nsteps * lo.B, 256)), dim3(256), 0, st, seed, first_step,
                     nsteps, nslots, lo.B, (unsigned long long)n_rows, idx);
  const long per = (long)lo.B * lo.A2;
  hipLaunchKernelGGL(vae_draw_eps_kernel, dim3(vae_blocks(nsteps * per, 256)), dim3(256), 0, st, seed ^ VAE_KEY_EPS,
                     first_step, nsteps, nslots, per, eps);
  OSA_CHECK_LAUNCH();
  return OSA_OK;
}

int osa_vae_step(const osa_vae_desc* desc, const osa_vae_hparams* hp, const osa_vae_state* s, const osa_crr_data* data,
                 const osa_vae_draw_buffers* dr, float* stats, float* ws, size_t ws_floats, int nsteps, void* stream) {
  VLayout lo;
  OSA_REQUIRE(desc && hp && s && data && dr && stats && ws && nsteps >= 1);
  const int rc0 = vae_make_layout(desc, &lo);
  if (rc0 != OSA_OK) return rc0;
  OSA_REQUIRE(hp->route == OSA_VAE_ROUTE_TILE || hp->route == OSA_VAE_ROUTE_SKINNY);
  if (hp->route == OSA_VAE_ROUTE_SKINNY && !vae_skinny_ok(lo)) return OSA_EUNSUPPORTED;
  const VWs w = vae_ws(lo);
  OSA_REQUIRE(ws_floats >= w.total && (reinterpret_cast<uintptr_t>(ws) & 15) == 0);
  OSA_REQUIRE(s->params && s->m && s->v && s->adam_step && s->step);
  OSA_REQUIRE(data->obs && data->act && data->n_rows >= 1 && data->ld_obs >= lo.D && data->ld_act >= lo.A);
  OSA_REQUIRE(dr->idx && dr->eps && dr->nslots >= 1);
  OSA_REQUIRE(hp->lr >= 0.f && hp->beta1 >= 0.0 && hp->beta1 < 1.0 && hp->beta2 >= 0.0 && hp->beta2 < 1.0);
  for (const float* p : {s->params, s->m, s->v}) OSA_REQUIRE((reinterpret_cast<uintptr_t>(p) & 15) == 0);
  VCtx c = {dr->idx, s->step, dr->nslots, lo.B, data->n_rows, hp->route == OSA_VAE_ROUTE_TILE, osa_stream(stream)};
  hipStream_t st = c.st;
  const int B = lo.B;
  const long P = (long)lo.e.P + lo.d.P;
  float *he[GM_MAXL], *hd[GM_MAXL];
  for (int l = 0; l < GM_MAXL; ++l) {
    he[l] = ws + w.he[l];
    hd[l] = ws + w.hd[l];
  }
  float* const dz[2] = {ws + w.dz[0], ws + w.dz[1]};
  const float* enc = s->params;
  const float* dec = s->params + lo.e.P;
  float* grad = ws + w.grad;
  // the two first-layer inputs: obs || act and obs || z, the dataset rows read through idx
  const SSrc xe = sk_concat(data->obs, data->ld_obs, 1, lo.D, data->act, data->ld_act, 1);
  const SSrc xd = sk_concat(data->obs, data->ld_obs, 1, lo.D, ws + w.z, lo.ld2a, 0);
  int rc;
  for (int it = 0; it < nsteps; ++it) {
    if ((rc = vae_forward(c, lo.e, lo.act, enc, xe, B, he, lo.e.ldh)) != OSA_OK) return rc;
    VHead hd_ = {he[lo.e.L - 1], dr->eps, s->step, ws + w.z, ws + w.sig, ws + w.msk, ws + w.red,
                 dr->nslots, B, lo.A2, lo.ld2a, lo.ld4a};
    hipLaunchKernelGGL(vae_enc_head_kernel, dim3(1), dim3(256), 0, st, hd_);
    if ((rc = vae_forward(c, lo.d, lo.act, dec, xd, B, hd, lo.d.ldh)) != OSA_OK) return rc;
    VLoss ls = {hd[lo.d.L - 1], data->act, dr->idx, s->step, ws + w.red, dz[0], stats, s->adam_step,
                dr->nslots, B, lo.A, lo.lda, data->ld_act, data->n_rows};
    hipLaunchKernelGGL(vae_dec_head_kernel, dim3(1), dim3(256), 0, st, ls);
    // the decoder's first-layer data gradient: the 2 A latent columns only
    if ((rc = vae_backward(c, lo.d, lo.act, dec, xd, hd, dz, grad + lo.e.P, ws + w.dzl, lo.D, lo.A2, lo.ld2a)) != OSA_OK)
      return rc;
    VHeadBwd hb = {he[lo.e.L - 1], dr->eps, ws + w.sig, ws + w.msk, ws + w.dzl, s->step, dz[0],
                   dr->nslots, B, lo.A2, lo.ld2a, lo.ld4a};
    hipLaunchKernelGGL(vae_head_bwd_kernel, dim3(vae_blocks((long)B * lo.ld4a, 256)), dim3(256), 0, st, hb);
    if ((rc = vae_backward(c, lo.e, lo.act, enc, xe, he, dz, grad, nullptr, 0, 0, 0)) != OSA_OK) return rc;
    hipLaunchKernelGGL(vae_adam_kernel, dim3(vae_blocks(P, 256)), dim3(256), 0, st, P, s->params, s->m, s->v, grad,
                       s->adam_step, s->step, hp->lr, hp->beta1, hp->beta2, hp->adam_eps);
    OSA_CHECK_LAUNCH();
  }
  return OSA_OK;
}

size_t osa_vae_decode_ws_floats(const osa_vae_desc* desc, long n) {
  VLayout lo;
  if (n < 1 || n > (1l << 20) || vae_make_layout(desc, &lo) != OSA_OK) return 0;
  return (size_t)n * (2 * (size_t)lo.d.maxldh + lo.ld2a);
}

int osa_vae_decode(const osa_vae_desc* desc, int route, const float* decoder, const float* obs, int ld_obs,
                   const float* z, int ld_z, long n, unsigned long long seed, unsigned long long offset, float* out,
                   int ld_out, float* ws, size_t ws_floats, void* stream) {
  VLayout lo;
  OSA_REQUIRE(desc && decoder && obs && out && ws && n >= 1);
  const int rc0 = vae_make_layout(desc, &lo);
  if (rc0 != OSA_OK) return rc0;
  if (n > (1l << 20)) return OSA_EUNSUPPORTED;
  OSA_REQUIRE(route == OSA_VAE_ROUTE_TILE || route == OSA_VAE_ROUTE_SKINNY);
  OSA_REQUIRE(ld_obs >= lo.D && ld_out >= lo.A && (!z || ld_z >= lo.A2));
  OSA_REQUIRE(ws_floats >= osa_vae_decode_ws_floats(desc, n) && (reinterpret_cast<uintptr_t>(ws) & 15) == 0);
  OSA_REQUIRE((reinterpret_cast<uintptr_t>(decoder) & 15) == 0);
  hipStream_t st = osa_stream(stream);
  float* hbuf[2] = {ws, ws + (size_t)n * lo.d.maxldh};
  float* zbuf = ws + 2 * (size_t)n * lo.d.maxldh;
  if (!z) {
    hipLaunchKernelGGL(vae_draw_z_kernel, dim3(vae_blocks(n * lo.ld2a, 256)), dim3(256), 0, st, seed, offset, n, lo.A2,
                       lo.ld2a, zbuf);
    z = zbuf;
    ld_z = lo.ld2a;
  }
  VCtx c = {nullptr, nullptr, 1, 0, 0, route == OSA_VAE_ROUTE_TILE, st};
  const SSrc x0 = sk_concat(obs, ld_obs, 0, lo.D, z, ld_z, 0);
  float* h[GM_MAXL];
  int ldh[GM_MAXL];
  for (int l = 0; l < lo.d.L; ++l) {
    const bool top = l + 1 == lo.d.L;
    h[l] = top ? out : hbuf[l & 1];
    ldh[l] = top ? ld_out : lo.d.ldh[l];
  }
  const int rc = vae_forward(c, lo.d, lo.act, decoder, x0, (int)n, h, ldh);
  if (rc != OSA_OK) return rc;
  OSA_CHECK_LAUNCH();
  return OSA_OK;
}

}  // extern "C"
