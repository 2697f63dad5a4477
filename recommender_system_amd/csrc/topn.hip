// topn.hip — DSSM retrieval: exact top-N by inner product, no [U, I] buffer.
//
//   rs_topn_inner_product  for every user row the N items with the largest
//                       score(u, i) = sum_k user[u, k] item[i, k], ordered by
//                       the KEY (score descending, item position ascending).
//
// The key is one 64-bit word: the score's bits mapped to an unsigned that
// orders like the float (high word), then ~position (low word) — "larger key"
// is "better", two keys are never equal, and 0 is "no item" (below every real
// key).  Every comparison below is on keys, so the result is a function of the
// scores alone: not of the split count, the queue order or the timing.
//
//   topn_partial_kernel  grid (user tiles of 64 rows) x (item splits).  The
//                       workgroup stages its 64 user rows in LDS (zero-padded
//                       to a k-group, as A in inbatch_softmax_tile); its 8
//                       waves walk the 16-item tiles of the split in rounds
//                       (round r: wave w takes tile 8 r + w).  A wave loads
//                       an item tile's B operand once per k-group (ib_load4)
//                       and feeds the four 16-row blocks: 4 MFMA chains, each
//                       one v_mfma_f32_16x16x4_f32 chain over the k-groups in
//                       ascending order — a pair's score is the same bits
//                       wherever it falls.  Each user row keeps its sorted
//                       best-N keys and the N-th (the threshold: its score
//                       and position) in LDS.  A lane compares its 16 scores
//                       with the rows' thresholds (two ds_read_b128 per row
//                       block: the key comparison, exactly); the few that
//                       pass are pushed as keys into the row's
//                       32-entry LDS queue (LDS atomic counter).  When a
//                       queue reaches 24, every row whose queue holds 8 or
//                       more is merged into its list, one wave per row, the
//                       waves side by side (ranks by counting: no sort
//                       network), and the thresholds tighten; a push that
//                       found its queue full is retried after the merge.
//                       One block barrier per round decides whether
//                       anything is to be merged.
//   topn_merge_kernel   one workgroup per user: the S sorted partial lists
//                       (keys, from the workspace, every slot written by the
//                       partial kernel) are merged pairwise in LDS, log2 S
//                       levels of binary-search ranking, and the N keys left
//                       are decoded.  S = 1
//                       writes the result from the partial kernel directly.
#include "dssm_softmax.hpp"

namespace rs {

typedef unsigned long long tn_key_t;
typedef int intx4 __attribute__((ext_vector_type(4)));

constexpr int TN_UT = 64;     // user rows per workgroup
constexpr int TN_NW = 8;      // waves per workgroup
constexpr int TN_QCAP = 32;   // queue entries per row
constexpr int TN_QHI = 24;    // a queue this full calls for a merge ...
constexpr int TN_QLO = 8;     // ... of every row whose queue holds this many: the waves merge rows side by side
constexpr int TN_MAXN = 128;  // two list entries per lane in the merge
constexpr int TN_MAXE = IB_MAXE;
constexpr int TN_MAXS = 64;   // splits: the merge kernel holds 1.5 S x N keys in LDS (96 KiB at most)
constexpr int TN_CUS = 256;   // the auto split aims at two workgroups per CU of an MI355X
constexpr size_t TN_LDS_MAX = 160 * 1024;

struct TopnArgs {
  const float* user;
  int64_t us;
  const float* item;
  int64_t is;
  int64_t U, I;
  int64_t tps;  // 16-item tiles per split
  int E, N, S, rsa, vec;
  int32_t* out_idx;
  float* out_score;
  tn_key_t* part;  // [S][U][N] keys (S > 1)
};

__device__ __forceinline__ tn_key_t tn_key(float s, int64_t pos) {
  const unsigned b = __float_as_uint(s + 0.0f);  // (-0 counts as +0)
  const unsigned o = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return (static_cast<tn_key_t>(o) << 32) | (0xFFFFFFFFu - static_cast<unsigned>(pos));
}
__device__ __forceinline__ float tn_score(tn_key_t k) {
  const unsigned o = static_cast<unsigned>(k >> 32);
  return k == 0 ? -INFINITY : __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
}
__device__ __forceinline__ int32_t tn_pos(tn_key_t k) {
  return k == 0 ? -1 : static_cast<int32_t>(0xFFFFFFFFu - static_cast<unsigned>(k));
}

// how many of the descending keys L[0 .. n) are larger than x
__device__ __forceinline__ int tn_count_greater(const tn_key_t* L, int n, tn_key_t x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (L[mid] > x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ tn_key_t tn_readlane(tn_key_t k, int i) {
  return (static_cast<tn_key_t>((unsigned)__builtin_amdgcn_readlane((int)(k >> 32), i)) << 32) |
         (unsigned)__builtin_amdgcn_readlane((int)k, i);
}

// One wave merges row u's queue into its list: every key's rank among list and
// queue together is counted (keys are distinct), and the keys of rank < N are
// written back at their rank.  The list sits in registers (two keys per lane),
// the queue one key per lane.  For queue key q_i, c_i = the number of list
// keys above it (two ballots); list key j moves down by the number of i with
// c_i <= j, and q_i lands at c_i + the number of queue keys above it.  The
// counting loop reads lanes, not LDS.  All LDS reads come before all writes:
// the wave's LDS instructions execute in order.
__device__ __forceinline__ void tn_flush_row(tn_key_t* L, tn_key_t* Q, int* qn, float* thrS, int* thrP, int N) {
  const int lane = threadIdx.x & 63;
  int m = __builtin_amdgcn_readfirstlane(*qn);
  if (m > TN_QCAP) m = TN_QCAP;
  const tn_key_t q = lane < m ? Q[lane] : 0;
  const tn_key_t l0 = lane < N ? L[lane] : 0, l1 = lane + 64 < N ? L[lane + 64] : 0;  // (0: below every queue key)
  int r0 = lane, r1 = lane + 64, rq = 0;
  for (int i = 0; i < m; ++i) {
    const tn_key_t qi = tn_readlane(q, i);
    const int ci = __popcll(__ballot(l0 > qi)) + __popcll(__ballot(l1 > qi));
    r0 += ci <= lane;
    r1 += ci <= lane + 64;
    rq += qi > q;
    if (lane == i) rq += ci;
  }
  __builtin_amdgcn_wave_barrier();
  auto put = [&](int r, tn_key_t k) {
    if (r < N) {
      L[r] = k;
      if (r == N - 1) {  // the row's new threshold (k = 0: the list is not full yet, everything passes)
        *thrS = tn_score(k);
        *thrP = k ? tn_pos(k) : 0x7fffffff;
      }
    }
  };
  if (lane < N) put(r0, l0);
  if (lane + 64 < N) put(r1, l1);
  if (lane < m) put(rq, q);
  if (lane == 0) *qn = 0;
}

__global__ __launch_bounds__(TN_NW * 64) void topn_partial_kernel(TopnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int N = a.N;
  float* A = smem;  // [TN_UT][rsa]
  tn_key_t* list = reinterpret_cast<tn_key_t*>(smem + TN_UT * a.rsa);  // [TN_UT][N], descending
  tn_key_t* queue = list + TN_UT * N;                                  // [TN_UT][TN_QCAP]
  float* thrS = reinterpret_cast<float*>(queue + TN_UT * TN_QCAP);     // [TN_UT] the score of the row's N-th key
  int* thrP = reinterpret_cast<int*>(thrS + TN_UT);                    // [TN_UT] ... and its position
  int* qn = thrP + TN_UT;                                              // [TN_UT] pushes since the last merge
  int* flag = qn + TN_UT;                                              // [3] "a queue is full enough" (see the loop)
  const int tid = threadIdx.x;
  const int lane = tid & 63, g = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t u0 = (int64_t)blockIdx.x * TN_UT;
  const int split = blockIdx.y;
  const int KG = (a.E + 15) >> 4;

  for (int r = w; r < TN_UT; r += TN_NW) {
    const int64_t u = u0 + r < a.U ? u0 + r : a.U - 1;
    for (int c = lane; c < 16 * KG; c += 64) A[r * a.rsa + c] = c < a.E ? a.user[u * a.us + c] : 0.f;
  }
  for (int i = tid; i < TN_UT * N; i += TN_NW * 64) list[i] = 0;
  if (tid < TN_UT) {
    const bool live = u0 + tid < a.U;  // a row past U takes nothing
    thrS[tid] = live ? -INFINITY : INFINITY;
    thrP[tid] = live ? 0x7fffffff : -1;
    qn[tid] = 0;
    if (tid < 3) flag[tid] = 0;
  }
  __syncthreads();

  const int64_t NT = (a.I + 15) >> 4;
  const int64_t t0 = split * a.tps, t1 = t0 + a.tps < NT ? t0 + a.tps : NT;
  const int rounds = (int)((t1 - t0 + TN_NW - 1) / TN_NW);  // the same for every wave
  const bool vec = a.vec != 0;
  auto row_of = [&](int64_t jt) {
    const int64_t j = jt * 16 + (lane & 15);
    return a.item + (j < a.I ? j : a.I - 1) * a.is;  // (a column past I re-reads the last row and is dropped)
  };
  const float* ap = A + (lane & 15) * a.rsa + 4 * g;

  // the first two k-groups of the next round's tile are fetched a round ahead
  const float* row = row_of(t0 + w);
  floatx4 pre0 = ib_load4(row, 4 * g, a.E, vec), pre1 = ib_load4(row, 16 + 4 * g, a.E, vec);
  int fi = 0;
  for (int rd = 0; rd < rounds; ++rd) {
    const int64_t jt = t0 + (int64_t)rd * TN_NW + w;
    const int64_t j = jt * 16 + (lane & 15);
    const float* cur = row;
    const floatx4 b0 = pre0, b1 = pre1;
    if (rd + 1 < rounds) {
      row = row_of(jt + TN_NW);
      pre0 = ib_load4(row, 4 * g, a.E, vec);
      pre1 = ib_load4(row, 16 + 4 * g, a.E, vec);
    }
    floatx4 acc[4];
    // bit 4 rb + r: the score of user row 16 rb + 4 g + r beats that row's threshold — exactly the key
    // comparison (score, then the lower position), on one ds_read_b128 of scores and one of positions
    auto admit = [&]() {
      unsigned m = 0;
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) {
        const floatx4 th = *reinterpret_cast<const floatx4*>(thrS + rb * 16 + 4 * g);
        const intx4 tp = *reinterpret_cast<const intx4*>(thrP + rb * 16 + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (acc[rb][r] > th[r] || (acc[rb][r] == th[r] && (int)j < tp[r])) m |= 1u << (4 * rb + r);
      }
      return m;
    };
    unsigned pm = 0;  // bit 4 rb + r: the score of user row 16 rb + 4 g + r is still to be pushed
    if (jt < t1) {
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) acc[rb] = floatx4{0.f, 0.f, 0.f, 0.f};
      floatx4 bn = KG > 2 ? ib_load4(cur, 32 + 4 * g, a.E, vec) : b0;
      for (int q = 0; q < KG; ++q) {
        const floatx4 bv = q == 0 ? b0 : q == 1 ? b1 : bn;
        if (q >= 2 && q + 1 < KG) bn = ib_load4(cur, 16 * (q + 1) + 4 * g, a.E, vec);
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) {
          const floatx4 av = *reinterpret_cast<const floatx4*>(ap + rb * 16 * a.rsa + 16 * q);
#pragma unroll
          for (int t = 0; t < 4; ++t) acc[rb] = mfma16x16x4(av[t], bv[t], acc[rb]);
        }
      }
      if (j < a.I) pm = admit();
    }
    bool trig = false;
    for (;;) {
      if (pm) {
        // a row block at a time: its (up to four) counter atomics are in flight
        // together, then the keys go to the slots they returned
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) {
          int slot[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            slot[r] = 0;
            if (pm & (1u << (4 * rb + r))) slot[r] = atomicAdd(&qn[rb * 16 + 4 * g + r], 1);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const unsigned bit = 1u << (4 * rb + r);
            if (pm & bit) {
              if (slot[r] < TN_QCAP) {
                queue[(rb * 16 + 4 * g + r) * TN_QCAP + slot[r]] = tn_key(acc[rb][r], j);
                pm &= ~bit;
              }
              trig |= slot[r] >= TN_QHI - 1;  // (a full queue: the push stays pending)
            }
          }
        }
      }
      // the block-wide "or" of trig in one barrier: three flags in rotation — this
      // pass's is set before the barrier and read after it, and thread 0 clears
      // the one the NEXT pass but one will use (last read before this barrier)
      if (trig) flag[fi] = 1;
      __syncthreads();
      const int any = flag[fi];
      if (tid == 0) flag[fi == 0 ? 2 : fi - 1] = 0;
      fi = fi == 2 ? 0 : fi + 1;
      if (!any) break;
      for (int u = w; u < TN_UT; u += TN_NW)
        if (__builtin_amdgcn_readfirstlane(qn[u]) >= TN_QLO)
          tn_flush_row(list + u * N, queue + u * TN_QCAP, qn + u, thrS + u, thrP + u, N);
      __syncthreads();
      trig = false;
      if (pm) pm &= admit();  // what is still pending, against the tightened thresholds
    }
  }
  // what the queues still hold (the last barrier above made every push visible)
  for (int u = w; u < TN_UT; u += TN_NW)
    if (__builtin_amdgcn_readfirstlane(qn[u]) > 0)
      tn_flush_row(list + u * N, queue + u * TN_QCAP, qn + u, thrS + u, thrP + u, N);
  __syncthreads();
  for (int r = w; r < TN_UT; r += TN_NW) {
    const int64_t u = u0 + r;
    if (u >= a.U) break;
    for (int n = lane; n < N; n += 64) {
      const tn_key_t k = list[r * N + n];
      if (a.S > 1) {
        a.part[((int64_t)split * a.U + u) * N + n] = k;
      } else {
        a.out_idx[u * N + n] = tn_pos(k);
        a.out_score[u * N + n] = tn_score(k);
      }
    }
  }
}

// One workgroup per user: the S sorted lists are merged pairwise, level by
// level, between two LDS buffers — a key of list s at index j lands at j + the
// number of keys of list s ^ 1 above it (a binary search), if that is below N —
// until one list is left.  S = 0: nothing to merge, every slot is padding.
constexpr int TN_MT = 256;
__global__ __launch_bounds__(TN_MT) void topn_merge_kernel(const tn_key_t* __restrict__ part, int64_t U, int N, int S,
                                                           int32_t* __restrict__ out_idx,
                                                           float* __restrict__ out_score) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  tn_key_t* src = reinterpret_cast<tn_key_t*>(smem);  // [S][N]
  tn_key_t* dst = src + S * N;                        // [(S + 1) / 2][N]
  const int tid = threadIdx.x;
  const int64_t u = blockIdx.x;
  for (int e = tid; e < S * N; e += TN_MT) {
    const int s = e / N;
    src[e] = part[((int64_t)s * U + u) * N + (e - s * N)];
  }
  __syncthreads();
  int L = S;
  while (L > 1) {
    const int H = (L + 1) >> 1;
    for (int e = tid; e < H * N; e += TN_MT) dst[e] = 0;
    __syncthreads();
    for (int e = tid; e < L * N; e += TN_MT) {
      const tn_key_t k = src[e];
      if (k == 0) continue;
      const int s = e / N, j = e - s * N, o = s ^ 1;
      const int rank = o < L ? j + tn_count_greater(src + o * N, N, k) : j;
      if (rank < N) dst[(s >> 1) * N + rank] = k;
    }
    __syncthreads();
    tn_key_t* t = src;
    src = dst;
    dst = t;
    L = H;
  }
  for (int n = tid; n < N; n += TN_MT) {
    const tn_key_t k = L ? src[n] : 0;
    out_idx[u * N + n] = tn_pos(k);
    out_score[u * N + n] = tn_score(k);
  }
}

// ---- host side
static int tn_rsa(int E) { return ((E + 15) / 16 * 16 + 63) / 64 * 64 + 8; }
static size_t tn_lds(int E, int N) {
  return (size_t)TN_UT * tn_rsa(E) * sizeof(float) + (size_t)TN_UT * (N + TN_QCAP) * sizeof(tn_key_t) +
         (size_t)TN_UT * (sizeof(float) + 2 * sizeof(int)) + 16;
}
static bool tn_ok(int E, int N) {
  return E >= 1 && E <= TN_MAXE && N >= 1 && N <= TN_MAXN && tn_lds(E, N) <= TN_LDS_MAX;
}

// the split count in effect and the tiles per split: no split is empty
static int tn_splits(int64_t U, int64_t I, int item_splits, int64_t& tps) {
  const int64_t NT = (I + 15) / 16;
  tps = NT;
  if (NT <= 1) return 1;
  int64_t S = item_splits;
  if (S <= 0) {  // two workgroups per CU, at least eight rounds of tiles per split
    const int64_t ut = U > 0 ? (U + TN_UT - 1) / TN_UT : 1;
    S = (2 * TN_CUS + ut - 1) / ut;
    const int64_t most = NT / (8 * TN_NW);
    if (S > most) S = most;
  }
  if (S > TN_MAXS) S = TN_MAXS;
  if (S > NT) S = NT;
  if (S < 1) S = 1;
  tps = (NT + S - 1) / S;
  return (int)((NT + tps - 1) / tps);
}

}  // namespace rs

using namespace rs;

extern "C" int rs_topn_inner_product_ok(int E, int N) { return tn_ok(E, N) ? 1 : 0; }

extern "C" int64_t rs_topn_inner_product_workspace_size(int64_t U, int64_t I, int N, int item_splits) {
  if (U < 0 || I < 0 || N < 1 || item_splits < 0) return -1;
  int64_t tps;
  const int S = tn_splits(U, I, item_splits, tps);
  return S > 1 ? (int64_t)S * U * N * (int64_t)sizeof(tn_key_t) : 0;
}

extern "C" int rs_topn_inner_product(const float* user, int64_t user_stride, int64_t U, const float* item,
                                     int64_t item_stride, int64_t I, int E, int N, int item_splits, int32_t* out_idx,
                                     float* out_score, void* workspace, int64_t workspace_bytes, rs_stream_t stream) {
  const char* what = "rs_topn_inner_product";
  RS_REQUIRE(U >= 0 && I >= 0, "%s: negative U / I", what);
  RS_REQUIRE(N >= 1, "%s: N must be at least 1", what);
  RS_REQUIRE(item_splits >= 0, "%s: negative item_splits", what);
  RS_REQUIRE(tn_ok(E, N),
             "%s: shape not supported (rs_topn_inner_product_ok: E 1..%d, N 1..%d, the tile's LDS <= 160 KiB)", what,
             TN_MAXE, TN_MAXN);
  RS_REQUIRE(user_stride >= E && item_stride >= E, "%s: bad stride", what);
  RS_REQUIRE(I < (1ll << 31), "%s: too many items", what);
  if (U == 0) return RS_OK;
  RS_REQUIRE(out_idx && out_score, "%s: null output", what);
  RS_REQUIRE(U * (int64_t)N < (1ll << 40), "%s: U too large", what);
  hipStream_t st = as_stream(stream);
  if (I == 0) {
    RS_REQUIRE(U < (1ll << 31), "%s: U too large", what);
    topn_merge_kernel<<<(unsigned)U, TN_MT, 0, st>>>(nullptr, U, N, 0, out_idx, out_score);
    return launch_status(what);
  }
  RS_REQUIRE(user && item, "%s: null pointer", what);
  TopnArgs a{};
  a.S = tn_splits(U, I, item_splits, a.tps);
  const int64_t need = a.S > 1 ? (int64_t)a.S * U * N * (int64_t)sizeof(tn_key_t) : 0;
  RS_REQUIRE(need == 0 || (workspace && workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0),
             "%s: the workspace needs %lld bytes (8-byte aligned)", what, (long long)need);
  const int64_t ut = (U + TN_UT - 1) / TN_UT;
  RS_REQUIRE(ut < (1ll << 31) && U < (1ll << 31), "%s: U too large", what);
  a.user = user;
  a.us = user_stride;
  a.item = item;
  a.is = item_stride;
  a.U = U;
  a.I = I;
  a.E = E;
  a.N = N;
  a.rsa = tn_rsa(E);
  a.vec = E % 4 == 0 && item_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(item) & 15) == 0;
  a.out_idx = out_idx;
  a.out_score = out_score;
  a.part = static_cast<tn_key_t*>(workspace);
  launch_lds<topn_partial_kernel>(dim3((unsigned)ut, (unsigned)a.S), TN_NW * 64, tn_lds(E, N), st, a);
  int rc = launch_status(what);
  if (rc != RS_OK || a.S == 1) return rc;
  launch_lds<topn_merge_kernel>((unsigned)U, TN_MT, (size_t)(a.S + (a.S + 1) / 2) * N * sizeof(tn_key_t), st,
                                static_cast<const tn_key_t*>(a.part), U, N, a.S, out_idx, out_score);
  return launch_status(what);
}
