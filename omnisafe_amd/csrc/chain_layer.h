// The row-resident layer of the fused chain kernels (bcq_kernels.hip: bcq_chain_kernel; td3_kernels.hip:
// td3_forward_kernel): a workgroup of four waves carries 32 rows through every layer of a network with the activations
// in LDS and the weights straight from global memory into the MFMAs.  Moved here unchanged from bcq_kernels.hip; both
// translation units include it and get their own instantiations.
#pragma once
#include "crr_layers.h"

namespace {

constexpr int BC_ROWS = 32;            // rows of a workgroup = the MFMA tile's
constexpr int BC_MAXW = 256;           // widest hidden layer the LDS buffers take
constexpr int BC_LDH = BC_MAXW + 4;    // leading dimension of an activation buffer
constexpr int BC_PART = 4 * 16 * 64;   // the four waves' partial tiles of a K-split layer
constexpr int BC_LDS_DYN = 160 * 1024 - 1024;  // the CU's 160 KB less the kernel's static table of the three networks

// a network as the kernel walks it
struct BNetK {
  int L, act;
  int N[GM_MAXL], ld[GM_MAXL], oW[GM_MAXL], ob[GM_MAXL];
};
BNetK bcq_netk(const CNet& n) {
  BNetK k = {};
  k.L = n.L; k.act = n.act;
  for (int l = 0; l < n.L; ++l) {
    k.N[l] = n.out[l]; k.ld[l] = n.ld[l]; k.oW[l] = n.oW[l]; k.ob[l] = n.ob[l];
  }
  return k;
}

// One layer over the workgroup's 32 rows: emit(row, n, sum_k src[row][k] W[n][k] + bias[n]) for every column n of the
// tiles that cover N (n >= N: the sum is 0).  src: LDS rows of lds floats, finite up to column ldw = K rounded to 4.
// Ends with a barrier: what emit wrote is visible, src and part are free.
template <class Emit>
__device__ __forceinline__ void bc_layer(const float* __restrict__ W, const float* __restrict__ bias, int N, int ldw,
                                         const float* src, int lds, float* part, Emit emit) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, kk = lane >> 5;
  const int nks = (ldw + 7) >> 3;  // K steps of 8: lane group kk consumes k = 8 s + 4 kk + q in MFMA step q
  const float* arow = src + l31 * lds + 4 * kk;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  if (N > 32) {
    if (32 * wave < N) {  // tiles wave and wave + 4 (wave-uniform)
      const bool two = 32 * (wave + 4) < N;
      const int na = 32 * wave + l31, nb = na + 128;
      const bool oka = na < N, okb = two && nb < N;
      const float* wa = W + (long)na * ldw + 4 * kk;
      const float* wb = W + (long)nb * ldw + 4 * kk;
      f32x16 acc0, acc1;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
      f32x4 cur[2][4], nxt[2][4];
      auto fetch = [&](f32x4(&w)[2][4], int kc) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = 8 * (kc + j);
          const bool in = k + 4 * kk < ldw;
          w[0][j] = (oka && in) ? *reinterpret_cast<const f32x4*>(wa + k) : zero;
          w[1][j] = (okb && in) ? *reinterpret_cast<const f32x4*>(wb + k) : zero;
        }
      };
      fetch(cur, 0);
      for (int kc = 0; kc < nks; kc += 4) {
        const bool more = kc + 4 < nks;
        if (more) fetch(nxt, kc + 4);  // in flight under this block's MFMAs
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = 8 * (kc + j);
          const f32x4 af = k + 4 * kk < ldw ? *reinterpret_cast<const f32x4*>(arow + k) : zero;
#pragma unroll
          for (int q = 0; q < 4; ++q) acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(af[q], cur[0][j][q], acc0, 0, 0, 0);
          if (two) {
#pragma unroll
            for (int q = 0; q < 4; ++q) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(af[q], cur[1][j][q], acc1, 0, 0, 0);
          }
        }
        if (more) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            cur[0][j] = nxt[0][j];
            cur[1][j] = nxt[1][j];
          }
        }
      }
      const float ba = oka ? bias[na] : 0.f, bb = okb ? bias[nb] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * kk;  // D[row][col = l31] of the 32 x 32 MFMA
        emit(row, na, acc0[r] + ba);
        if (two) emit(row, nb, acc1[r] + bb);
      }
    }
  } else {  // one tile: K split over the waves, the partial tiles added in wave order
    const int per = (nks + 3) >> 2, s0 = wave * per, s1 = s0 + per < nks ? s0 + per : nks;
    const bool ok = l31 < N;
    const float* wr = W + (long)l31 * ldw + 4 * kk;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int s = s0; s < s1; ++s) {
      const int k = 8 * s;
      const bool in = k + 4 * kk < ldw;
      const f32x4 af = in ? *reinterpret_cast<const f32x4*>(arow + k) : zero;
      const f32x4 bf = (ok && in) ? *reinterpret_cast<const f32x4*>(wr + k) : zero;
#pragma unroll
      for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[q], bf[q], acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) part[(wave * 16 + r) * 64 + lane] = acc[r];
    __syncthreads();
    const float b = ok ? bias[l31] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = 4 * wave + i;
      float v = part[(0 * 16 + r) * 64 + lane];
      v += part[(1 * 16 + r) * 64 + lane];
      v += part[(2 * 16 + r) * 64 + lane];
      v += part[(3 * 16 + r) * 64 + lane];
      emit((r & 3) + 8 * (r >> 2) + 4 * kk, l31, v + b);
    }
  }
  __syncthreads();
}

// hidden layer: activation into the other ping-pong buffer, its padding columns written zero
struct BEmitHidden {
  float* dst;
  int N, act;
  __device__ __forceinline__ void operator()(int row, int n, float v) const {
    if (n < N) dst[row * BC_LDH + n] = gm_act(v, act);
    else if (n < ((N + 3) & ~3)) dst[row * BC_LDH + n] = 0.f;
  }
};

// a network over the block's rows: layer 0 reads xin, layer l > 0 the buffer layer l - 1 wrote; `top` takes the head
template <class Top>
__device__ __forceinline__ void bc_net(const BNetK* nk, const float* __restrict__ p, const float* xin, int ldxin,
                                       float* hb0, float* hb1, float* part, Top top) {
  const int L = __builtin_amdgcn_readfirstlane(nk->L), act = __builtin_amdgcn_readfirstlane(nk->act);
  for (int l = 0; l < L; ++l) {
    const int N = __builtin_amdgcn_readfirstlane(nk->N[l]), ld = __builtin_amdgcn_readfirstlane(nk->ld[l]);
    const float* W = p + __builtin_amdgcn_readfirstlane(nk->oW[l]);
    const float* b = p + __builtin_amdgcn_readfirstlane(nk->ob[l]);
    const float* src = l == 0 ? xin : ((l & 1) ? hb0 : hb1);
    const int lds = l == 0 ? ldxin : BC_LDH;
    if (l + 1 < L) bc_layer(W, b, N, ld, src, lds, part, BEmitHidden{(l & 1) ? hb1 : hb0, N, act});
    else bc_layer(W, b, N, ld, src, lds, part, top);
  }
}

}  // namespace
