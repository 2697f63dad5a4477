// dssm_softmax.hpp — the in-batch softmax's tile walk, shared by
// rs_inbatch_softmax_fwd (dssm.hip) and rs_inbatch_softmax_train_fwd
// (dssm_train.hip, which also keeps logsumexp per row for the backward): one
// device function, so the two losses are the same bits by construction.
#pragma once
#include "concat.hpp"
#include "mlp_tower.hpp"

namespace rs {

__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

constexpr int IB_NW = 16;
constexpr int IB_MAXE = 512;
constexpr float IB_NEG = -3.0e38f;  // "no column yet": exp(IB_NEG - m) = 0 for any finite m

struct IbsArgs {
  const float* user;
  int64_t us;
  const float* item;
  int64_t is;
  const void* idx;
  int idx_kind;
  const float* logq;
  int64_t n_items;
  float temp;
  float* loss;
  int64_t B;
  int E, rsa, vec;
  int* err;
  float* lse;  // [B] logsumexp_j z_ij (the training forward), else unused
};

// item[row][k .. k + 3], zeros past E
__device__ __forceinline__ floatx4 ib_load4(const float* row, int k, int E, bool vec) {
  floatx4 v = {0.f, 0.f, 0.f, 0.f};
  if (vec) {
    if (k < E) v = *reinterpret_cast<const floatx4*>(row + k);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (k + j < E) v[j] = row[k + j];
  }
  return v;
}

// (m, s) <- the two partial softmax sums merged: max m, sum of exp(z - m)
__device__ __forceinline__ void ib_merge(float& m, float& s, float m2, float s2) {
#pragma clang fp contract(off)
  const float mn = fmaxf(m, m2);
  s = s * expf(m - mn) + s2 * expf(m2 - mn);
  m = mn;
}

// The whole workgroup's work (IB_NW waves, dynamic LDS of ib_lds bytes).
// LSE: also a.lse[i] = M + log S, the number the loss subtracts z_ii from.
template <bool LSE>
__device__ __forceinline__ void inbatch_softmax_tile(const IbsArgs& a) {
  extern __shared__ float smem[];
  float* A = smem;                    // [16][rsa]: u / temperature, zero-padded to a k-group
  float* part = smem + 16 * a.rsa;    // [IB_NW][16][2]
  float* diag = part + IB_NW * 32;    // [16]
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t i0 = (int64_t)blockIdx.x * 16;
  const int KG = (a.E + 15) >> 4;
  {
    const int64_t i = i0 + w < a.B ? i0 + w : a.B - 1;
    for (int c = lane; c < 16 * KG; c += 64) A[w * a.rsa + c] = c < a.E ? a.user[i * a.us + c] / a.temp : 0.f;
  }
  __syncthreads();
  float m[4], s[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m[r] = IB_NEG;
    s[r] = 0.f;
  }
  const int64_t NT = (a.B + 15) >> 4;
  const float* ap = A + (lane & 15) * a.rsa + 4 * (lane >> 4);
  bool bad = false;
  for (int64_t jt = w; jt < NT; jt += IB_NW) {
    const int64_t j = jt * 16 + (lane & 15);
    const int64_t jc = j < a.B ? j : a.B - 1;
    const float* row = a.item + jc * a.is;
    // log Q of this lane's column (an index out of range: 0, flagged)
    int64_t id;
    const bool ok = a.idx_kind == RS_ID_I64 ? cc_id<1>(a.idx, jc, a.n_items, id) : cc_id<0>(a.idx, jc, a.n_items, id);
    const float lq = ok ? a.logq[id] : 0.f;
    bad |= !ok && j < a.B;
    MacAcc<4> acc;
    for (int q = 0; q < KG; ++q) {
      const floatx4 av = *reinterpret_cast<const floatx4*>(ap + 16 * q);
      const floatx4 bv = ib_load4(row, 16 * q + 4 * (lane >> 4), a.E, a.vec != 0);
      acc.mac4(av, bv);
    }
    const floatx4 dsum = acc.sum();
    if (j < a.B) {  // columns past B are excluded
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float z = dsum[r] - lq;
        ib_merge(m[r], s[r], z, 1.0f);
        if (jt == blockIdx.x && (lane & 15) == 4 * (lane >> 4) + r) diag[lane & 15] = z;
      }
    }
  }
  if (__any(bad) && lane == 0) flag_error(a.err);
  // the 16 lanes of a row (xor butterfly inside the DPP row), then the waves in wave order
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) {
      const float m2 = __shfl_xor(m[r], o), s2 = __shfl_xor(s[r], o);
      ib_merge(m[r], s[r], m2, s2);
    }
    if ((lane & 15) == 0) {
      const int row = 4 * (lane >> 4) + r;
      part[(w * 16 + row) * 2] = m[r];
      part[(w * 16 + row) * 2 + 1] = s[r];
    }
  }
  __syncthreads();
  if (threadIdx.x < 16 && i0 + threadIdx.x < a.B) {
    const int row = threadIdx.x;
    float M = IB_NEG;
    for (int p = 0; p < IB_NW; ++p) M = fmaxf(M, part[(p * 16 + row) * 2]);
    float S = 0.f;
    for (int p = 0; p < IB_NW; ++p) S += part[(p * 16 + row) * 2 + 1] * expf(part[(p * 16 + row) * 2] - M);
    const float lse = M + logf(S);
    a.loss[i0 + row] = lse - diag[row];
    if constexpr (LSE) a.lse[i0 + row] = lse;
  }
}

// ---- host side: the argument checks and geometry of both entries
inline int ib_fill(const char* what, const float* user, int64_t user_stride, const float* item, int64_t item_stride,
                   const void* item_idx, int idx_kind, const float* logq, int64_t n_items, float temperature,
                   float* loss, int64_t batch, int E, int* err_flag, IbsArgs& a) {
  RS_REQUIRE(batch >= 0, "%s: negative batch", what);
  RS_REQUIRE(E >= 1 && E <= IB_MAXE, "%s: E must be 1..%d", what, IB_MAXE);
  RS_REQUIRE(user_stride >= E && item_stride >= E && n_items >= 1, "%s: bad stride / n_items", what);
  RS_REQUIRE(idx_kind == RS_ID_I32 || idx_kind == RS_ID_I64, "%s: item_idx is int32 or int64", what);
  RS_REQUIRE(temperature > 0.f, "%s: temperature must be positive", what);
  if (batch == 0) return RS_OK;
  RS_REQUIRE(user && item && item_idx && logq && loss, "%s: null pointer", what);
  RS_REQUIRE((batch + 15) / 16 < (1ll << 31), "%s: batch too large", what);
  a.user = user;
  a.us = user_stride;
  a.item = item;
  a.is = item_stride;
  a.idx = item_idx;
  a.idx_kind = idx_kind;
  a.logq = logq;
  a.n_items = n_items;
  a.temp = temperature;
  a.loss = loss;
  a.B = batch;
  a.E = E;
  a.rsa = ((E + 15) / 16 * 16 + 63) / 64 * 64 + 8;
  a.vec = E % 4 == 0 && item_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(item) & 15) == 0;
  a.err = err_flag;
  a.lse = nullptr;
  return RS_OK;
}
inline int64_t ib_grid(const IbsArgs& a) { return (a.B + 15) / 16; }
inline size_t ib_lds(const IbsArgs& a) { return (size_t)(16 * a.rsa + IB_NW * 32 + 16) * sizeof(float); }

}  // namespace rs
