// metrics.hip — on-device evaluation metrics for the binary CTR models: the
// reference's scripts end with accuracy_score(y_test, [p > 0.5]) (model/fm.py:
// 38, deepFM.py:51, dcn.py:50, din.py:116, pnn.py:89, fnn.py:70-71; compile_fit
// asks Keras for metrics=['accuracy'], utils/compile_fit.py:13), two of them
// under the label "AUC".
//
// rs_binary_metrics: log-loss (Keras' probability form, as rs_bce_prob_grad,
//   but in fp64), accuracy counts and input checks in two launches: per-
//   workgroup partials in a fixed tree, then one workgroup over the partials
//   in index order.  No floating-point atomics: bit-identical run to run.
// rs_auc: exact, tie-aware ROC AUC of any finite fp32 scores and, with group
//   ids, the impression-weighted GAUC of the DIN paper.
//     keys     score -> order-preserving u32 (-0.0 == +0.0), value = sample
//              index (31 bits: n < 2^31) with label == 1 in bit 31, so the
//              sorted sequence carries its labels and nothing gathers them
//     sort     rs::sort_pairs_u32, 32 bits (stable)
//     flags    in sorted order: the label bit, tie-run head (key differs
//              from its left neighbour)
//     scans    rs::inclusive_sum_i32 of the positives and of the heads (the
//              negatives before position i are i - positives: no third scan)
//     starts   run r's first position, scattered by run id
//     runs     one thread per tie run: p_r, n_r and below_r (negatives in the
//              lower runs) from the scans at the run's two ends, p_r (2
//              below_r + n_r) summed over a workgroup's runs (at most
//              MT_MAXB workgroups stride over them) and added to U2 with one
//              int64 atomic each (integer addition: exact and order-free)
//   auc = U2 / (2 P Q).  GAUC: the score-sorted sequence is sorted again,
//   stably, by group id (ceil(log2(n_groups)) bits), heads are group heads or
//   key changes, below_r counts from the group's start, U2_g goes to the
//   group's int64 (one atomic per wave when the wave's runs share a group),
//   P_g and Q_g come from the scan at the group's two ends, one thread per
//   group computes size_g U2_g / (2 P_g Q_g) in fp64 and the terms are
//   reduced in a fixed order.
// No thread walks a run or a group and no workgroup waits on another: every
// dependency is a launch boundary.
#include "radix_sort.hpp"
#include "rs_common.hpp"

namespace rs {

constexpr int MT_T = 256;            // threads per workgroup
constexpr int MT_MAXB = 1024;        // partial-sum workgroups at most
constexpr int64_t MT_NMAX = 1ll << 31;
constexpr uint32_t AU_IDX = 0x7fffffffu;  // sample index of a sort value; bit 31: label == 1

static int64_t mt_al(int64_t x) { return (x + 255) / 256 * 256; }

// Fixed-order sum of v over the workgroup (MT_T threads); thread 0 gets it.
template <class T>
__device__ __forceinline__ T mt_block_sum(T v, T* red) {
  red[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int s = MT_T / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const T r = red[0];
  __syncthreads();
  return r;
}

// ---------------------------------------------------------- binary metrics
// partial record of one workgroup: n_pos, n_correct, n_bad_label, n_nan_pred
// (int64) and loss_sum (fp64), 5 words of 8 bytes padded to 8
constexpr int BM_W = 8;

static int bm_blocks(int64_t n) {
  const int64_t nb = (n + MT_T * 8 - 1) / (MT_T * 8);
  return (int)(nb < 1 ? 1 : nb > MT_MAXB ? MT_MAXB : nb);
}

__global__ __launch_bounds__(MT_T) void bm_partial(const float* __restrict__ pred, int64_t ldp,
                                                   const float* __restrict__ y, int64_t n,
                                                   unsigned long long* __restrict__ part) {
  __shared__ long long redi[MT_T];
  __shared__ double redd[MT_T];
  long long npos = 0, ncor = 0, nbad = 0, nnan = 0;
  double loss = 0.0;
  const double eps = 1e-7;
  // a thread's samples in index order: the workgroup's sum is a fixed tree
  for (int64_t i = (int64_t)blockIdx.x * MT_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * MT_T) {
    const float pf = pred[i * ldp], yf = y[i];
    const bool pos = yf == 1.0f;
    const bool nan = pf != pf;
    npos += pos;
    nbad += !(pos || yf == 0.0f);
    nnan += nan;
    ncor += (pf > 0.5f) == pos;
    const double p = (double)pf, t = (double)yf;
    const double q = fmin(fmax(p, eps), 1.0 - eps);
    const double term = -(t * log(q + eps) + (1.0 - t) * log(1.0 - q + eps));
    loss += nan ? 0.0 : term;
  }
  npos = mt_block_sum(npos, redi);
  ncor = mt_block_sum(ncor, redi);
  nbad = mt_block_sum(nbad, redi);
  nnan = mt_block_sum(nnan, redi);
  loss = mt_block_sum(loss, redd);
  if (threadIdx.x == 0) {
    unsigned long long* o = part + (int64_t)blockIdx.x * BM_W;
    o[0] = (unsigned long long)npos;
    o[1] = (unsigned long long)ncor;
    o[2] = (unsigned long long)nbad;
    o[3] = (unsigned long long)nnan;
    o[4] = (unsigned long long)__double_as_longlong(loss);
  }
}

__global__ __launch_bounds__(MT_T) void bm_final(const unsigned long long* __restrict__ part, int nb, int64_t n,
                                                 int accumulate, unsigned long long* __restrict__ result) {
  __shared__ long long redi[MT_T];
  __shared__ double redd[MT_T];
  long long v[4] = {0, 0, 0, 0};
  double loss = 0.0;
  for (int b = threadIdx.x; b < nb; b += MT_T) {
    const unsigned long long* p = part + (int64_t)b * BM_W;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] += (long long)p[j];
    loss += __longlong_as_double((long long)p[4]);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = mt_block_sum(v[j], redi);
  loss = mt_block_sum(loss, redd);
  if (threadIdx.x == 0) {
    long long r[8] = {(long long)n, v[0], v[1], 0, v[2], v[3], 0, 0};
    double l = loss;
    if (accumulate) {
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] += (long long)result[j];
      l = __longlong_as_double((long long)result[3]) + loss;
    }
    r[3] = __double_as_longlong(l);
#pragma unroll
    for (int j = 0; j < 8; ++j) result[j] = (unsigned long long)r[j];
  }
}

// -------------------------------------------------------------------- AUC
// result words (8 bytes each)
enum { AU_N = 0, AU_P, AU_Q, AU_U2, AU_AUC, AU_NAN, AU_FLAGS, AU_BADLABEL, AU_GAUC, AU_GUSED, AU_IUSED, AU_WORDS = 16 };
// device counters in the workspace (int64 each)
enum { AC_U2 = 0, AC_NAN, AC_BADLABEL, AC_FLAGS, AC_WORDS = 8 };
// per-workgroup record of the group-term reduction: term sum (fp64), groups, impressions
constexpr int GT_W = 4;

struct AucWs {
  int64_t cnt, key0, a, b, idx1, idx2, cpos, chead, start, sort, scan, gu2, gstart, gend, gpart, total;
};
static int gt_blocks(int64_t G) {
  const int64_t nb = (G + MT_T - 1) / MT_T;
  return (int)(nb < 1 ? 1 : nb > MT_MAXB ? MT_MAXB : nb);
}
static AucWs auc_ws(int64_t n, int64_t G) {
  AucWs w{};
  const int64_t m = n > 0 ? n : 1;
  int64_t o = 0;
  w.cnt = o; o = mt_al(o + AC_WORDS * 8);
  w.key0 = o; o = mt_al(o + m * 4);   // keys in sample order
  w.a = o; o = mt_al(o + m * 4);      // sort values (sample | label bit), then group keys in score order
  w.b = o; o = mt_al(o + m * 4);      // sorted keys, then sorted group keys
  w.idx1 = o; o = mt_al(o + m * 4);   // samples in score order
  w.cpos = o; o = mt_al(o + m * 4);
  w.chead = o; o = mt_al(o + m * 4);
  w.start = o; o = mt_al(o + m * 4);
  w.sort = o; o = mt_al(o + sort_pairs_ws_bytes(m));
  w.scan = o; o = mt_al(o + scan_ws_bytes(m));
  if (G > 0) {
    w.idx2 = o; o = mt_al(o + m * 4);  // samples in (group, score) order
    w.gu2 = o; o = mt_al(o + G * 8);
    w.gstart = o; o = mt_al(o + G * 4);
    w.gend = o; o = mt_al(o + G * 4);
    w.gpart = o; o = mt_al(o + (int64_t)gt_blocks(G) * GT_W * 8);
  }
  w.total = o;
  return w;
}

__device__ __forceinline__ uint32_t auc_key(float f, bool& nan) {
  uint32_t u = __float_as_uint(f);
  if ((u << 1) == 0u) u = 0u;  // -0.0 ties with +0.0
  nan = (u & 0x7fffffffu) > 0x7f800000u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// zero the counters and the per-group accumulators; group spans start empty
__global__ __launch_bounds__(MT_T) void auc_init(long long* __restrict__ cnt, long long* __restrict__ gu2,
                                                 int32_t* __restrict__ gstart, int32_t* __restrict__ gend, int64_t G) {
  const int64_t i = (int64_t)blockIdx.x * MT_T + threadIdx.x;
  if (i < AC_WORDS) cnt[i] = 0;
  if (i < G) {
    gu2[i] = 0;
    gstart[i] = -1;
    gend[i] = -1;
  }
}

__global__ __launch_bounds__(MT_T) void auc_keys(const float* __restrict__ s, int64_t lds_, const float* __restrict__ y,
                                                 int64_t n, uint32_t* __restrict__ key, uint32_t* __restrict__ idx,
                                                 long long* __restrict__ cnt) {
  const int64_t i = (int64_t)blockIdx.x * MT_T + threadIdx.x;
  bool nan = false, bad = false;
  if (i < n) {
    key[i] = auc_key(s[i * lds_], nan);
    const float yf = y[i];
    idx[i] = (uint32_t)i | (yf == 1.0f ? ~AU_IDX : 0u);
    bad = !(yf == 1.0f || yf == 0.0f);
  }
  const unsigned long long mn = __builtin_amdgcn_ballot_w64(nan), mb = __builtin_amdgcn_ballot_w64(bad);
  if ((threadIdx.x & 63) == 0) {
    if (mn) atomicAdd(reinterpret_cast<unsigned long long*>(cnt + AC_NAN), (unsigned long long)__popcll(mn));
    if (mb) atomicAdd(reinterpret_cast<unsigned long long*>(cnt + AC_BADLABEL), (unsigned long long)__popcll(mb));
  }
}

// group key of the score-sorted sequence; an id outside [0, G) is flagged and
// read as group 0, so every later index stays in bounds
template <int KIND>
__global__ __launch_bounds__(MT_T) void auc_group_keys(const void* __restrict__ gid, int64_t G,
                                                       const uint32_t* __restrict__ idx1, int64_t n,
                                                       uint32_t* __restrict__ gkey, long long* __restrict__ cnt) {
  const int64_t i = (int64_t)blockIdx.x * MT_T + threadIdx.x;
  if (i >= n) return;
  int64_t g;
  if (!Ids<KIND>::decode(Ids<KIND>::load(gid, idx1[i] & AU_IDX), G, g))
    atomicOr(reinterpret_cast<unsigned long long*>(cnt + AC_FLAGS), (unsigned long long)RS_FLAG_BAD_ID);
  gkey[i] = (uint32_t)g;
}

// positives and run heads of the sorted sequence (idx: the sorted values,
// label in bit 31).  GROUPED: skey is the keys in sample order (gathered
// through idx; the left neighbour's key comes through LDS), gkey the sorted
// group keys, and the group's first and last positions are recorded.
template <bool GROUPED>
__global__ __launch_bounds__(MT_T) void auc_flags(const uint32_t* __restrict__ skey, const uint32_t* __restrict__ gkey,
                                                  const uint32_t* __restrict__ idx, int64_t n,
                                                  int32_t* __restrict__ pos, int32_t* __restrict__ head,
                                                  int32_t* __restrict__ gstart, int32_t* __restrict__ gend) {
  __shared__ uint32_t keys[MT_T + 1];
  const int64_t i = (int64_t)blockIdx.x * MT_T + threadIdx.x;
  const bool in = i < n;
  const uint32_t v = in ? idx[i] : 0u;
  if constexpr (GROUPED) {
    const uint32_t k = in ? skey[v & AU_IDX] : 0u;
    keys[threadIdx.x + 1] = k;
    if (threadIdx.x == 0) keys[0] = (in && i > 0) ? skey[idx[i - 1] & AU_IDX] : 0u;
    __syncthreads();
    if (!in) return;
    const uint32_t g = gkey[i];
    const bool ghead = i == 0 || gkey[i - 1] != g;
    head[i] = ghead || keys[threadIdx.x] != k;
    if (ghead) gstart[g] = (int32_t)i;
    if (i == n - 1 || gkey[i + 1] != g) gend[g] = (int32_t)i;
  } else {
    if (!in) return;
    head[i] = i == 0 || skey[i - 1] != skey[i];
  }
  pos[i] = (int32_t)(v >> 31);
}

__global__ __launch_bounds__(MT_T) void auc_run_starts(const int32_t* __restrict__ head_flag_scan, int64_t n,
                                                       int32_t* __restrict__ start) {
  const int64_t i = (int64_t)blockIdx.x * MT_T + threadIdx.x;
  if (i >= n) return;
  const int32_t h = head_flag_scan[i];
  if (i == 0 || head_flag_scan[i - 1] != h) start[h - 1] = (int32_t)i;  // 1 <= h <= n
}

// one thread per tie run; the workgroups stride over the runs
__global__ __launch_bounds__(MT_T) void auc_runs(const int32_t* __restrict__ cpos, const int32_t* __restrict__ chead,
                                                 const int32_t* __restrict__ start, int64_t n,
                                                 long long* __restrict__ cnt) {
  __shared__ long long red[MT_T];
  const int64_t R = chead[n - 1];
  long long c = 0;
  for (int64_t r = (int64_t)blockIdx.x * MT_T + threadIdx.x; r < R; r += (int64_t)gridDim.x * MT_T) {
    const int64_t s = start[r];
    const int64_t e = r + 1 < R ? (int64_t)start[r + 1] - 1 : n - 1;
    const int64_t pb = s > 0 ? cpos[s - 1] : 0;  // positives before the run
    const int64_t p = cpos[e] - pb, nr = (e - s + 1) - p;
    c += p * (2 * (s - pb) + nr);                // s - pb: negatives before the run
  }
  c = mt_block_sum(c, red);
  if (threadIdx.x == 0 && c != 0) atomicAdd(reinterpret_cast<unsigned long long*>(cnt + AC_U2), (unsigned long long)c);
}

// the same per group: below_r counts from the group's start, the sum goes to
// the group's int64 (one atomic for the wave when its runs share a group)
__global__ __launch_bounds__(MT_T) void auc_group_runs(const int32_t* __restrict__ cpos,
                                                       const int32_t* __restrict__ chead,
                                                       const int32_t* __restrict__ start, int64_t n,
                                                       const uint32_t* __restrict__ gkey,
                                                       const int32_t* __restrict__ gstart,
                                                       long long* __restrict__ gu2) {
  const int64_t r = (int64_t)blockIdx.x * MT_T + threadIdx.x;
  const int64_t R = chead[n - 1];
  long long c = 0;
  uint32_t g = 0xffffffffu;
  if (r < R) {
    const int64_t s = start[r];
    const int64_t e = r + 1 < R ? (int64_t)start[r + 1] - 1 : n - 1;
    const int64_t pb = s > 0 ? cpos[s - 1] : 0;
    const int64_t p = cpos[e] - pb, nr = (e - s + 1) - p;
    g = gkey[s];
    const int64_t gs = gstart[g];
    const int64_t below = (s - pb) - (gs - (gs > 0 ? cpos[gs - 1] : 0));  // negatives since the group's start
    c = p * (2 * below + nr);
  }
  const uint32_t g0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)g);
  if (__builtin_amdgcn_ballot_w64(g != g0) == 0ull) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0 && c != 0 && g0 != 0xffffffffu)
      atomicAdd(reinterpret_cast<unsigned long long*>(gu2 + g0), (unsigned long long)c);
  } else if (c != 0) {
    atomicAdd(reinterpret_cast<unsigned long long*>(gu2 + g), (unsigned long long)c);
  }
}

// workgroup b: groups [b * chunk, (b + 1) * chunk) in a fixed assignment
__global__ __launch_bounds__(MT_T) void auc_group_terms(const long long* __restrict__ gu2,
                                                        const int32_t* __restrict__ gstart,
                                                        const int32_t* __restrict__ gend,
                                                        const int32_t* __restrict__ cpos, int64_t G, int64_t chunk,
                                                        unsigned long long* __restrict__ gpart) {
  __shared__ long long redi[MT_T];
  __shared__ double redd[MT_T];
  const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < G ? lo + chunk : G;
  double term = 0.0;
  long long used = 0, imp = 0;
  for (int64_t g = lo + threadIdx.x; g < hi; g += MT_T) {
    const int64_t s = gstart[g], e = gend[g];
    if (s < 0) continue;
    const int64_t size = e - s + 1;
    const int64_t P = cpos[e] - (s > 0 ? cpos[s - 1] : 0), Q = size - P;
    if (P > 0 && Q > 0) {
      term += (double)size * ((double)gu2[g] / (2.0 * (double)P * (double)Q));
      used += 1;
      imp += size;
    }
  }
  term = mt_block_sum(term, redd);
  used = mt_block_sum(used, redi);
  imp = mt_block_sum(imp, redi);
  if (threadIdx.x == 0) {
    unsigned long long* o = gpart + (int64_t)blockIdx.x * GT_W;
    o[0] = (unsigned long long)__double_as_longlong(term);
    o[1] = (unsigned long long)used;
    o[2] = (unsigned long long)imp;
  }
}

// global AUC words (first pass); the group words are cleared
__global__ void auc_final(const long long* __restrict__ cnt, const int32_t* __restrict__ cpos, int64_t n,
                          unsigned long long* __restrict__ result) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const long long P = n > 0 ? cpos[n - 1] : 0, Q = n - P, U2 = n > 0 ? cnt[AC_U2] : 0;
  const double nanv = __longlong_as_double(0x7ff8000000000000ll);
  const double auc = (P > 0 && Q > 0) ? (double)U2 / (2.0 * (double)P * (double)Q) : nanv;
  for (int j = 0; j < AU_WORDS; ++j) result[j] = 0;
  result[AU_N] = (unsigned long long)n;
  result[AU_P] = (unsigned long long)P;
  result[AU_Q] = (unsigned long long)Q;
  result[AU_U2] = (unsigned long long)U2;
  result[AU_AUC] = (unsigned long long)__double_as_longlong(auc);
  result[AU_NAN] = (unsigned long long)cnt[AC_NAN];
  result[AU_BADLABEL] = (unsigned long long)cnt[AC_BADLABEL];
  result[AU_GAUC] = (unsigned long long)__double_as_longlong(nanv);
}

__global__ __launch_bounds__(MT_T) void auc_group_final(const unsigned long long* __restrict__ gpart, int nb,
                                                        const long long* __restrict__ cnt,
                                                        unsigned long long* __restrict__ result) {
  __shared__ long long redi[MT_T];
  __shared__ double redd[MT_T];
  double term = 0.0;
  long long used = 0, imp = 0;
  for (int b = threadIdx.x; b < nb; b += MT_T) {
    const unsigned long long* p = gpart + (int64_t)b * GT_W;
    term += __longlong_as_double((long long)p[0]);
    used += (long long)p[1];
    imp += (long long)p[2];
  }
  term = mt_block_sum(term, redd);
  used = mt_block_sum(used, redi);
  imp = mt_block_sum(imp, redi);
  if (threadIdx.x == 0) {
    const double nanv = __longlong_as_double(0x7ff8000000000000ll);
    result[AU_GAUC] = (unsigned long long)__double_as_longlong(imp > 0 ? term / (double)imp : nanv);
    result[AU_GUSED] = (unsigned long long)used;
    result[AU_IUSED] = (unsigned long long)imp;
    result[AU_FLAGS] = (unsigned long long)cnt[AC_FLAGS];
  }
}

}  // namespace rs

using namespace rs;

extern "C" int64_t rs_binary_metrics_workspace_size(int64_t n) {
  if (n < 0 || n >= MT_NMAX) {
    set_error("rs_binary_metrics_workspace_size: need 0 <= n < 2^31");
    return -1;
  }
  return mt_al((int64_t)bm_blocks(n) * BM_W * 8);
}

extern "C" int rs_binary_metrics(const float* pred, int64_t pred_stride, const float* labels, int64_t n,
                                 int accumulate, void* result, void* workspace, rs_stream_t stream) {
  RS_REQUIRE(n >= 0 && n < MT_NMAX, "rs_binary_metrics: need 0 <= n < 2^31");
  RS_REQUIRE(result && workspace, "rs_binary_metrics: null pointer");
  RS_REQUIRE(n == 0 || (pred && labels && pred_stride >= 1), "rs_binary_metrics: null pointer or pred_stride < 1");
  hipStream_t st = as_stream(stream);
  unsigned long long* part = static_cast<unsigned long long*>(workspace);
  const int nb = n > 0 ? bm_blocks(n) : 0;
  if (nb) bm_partial<<<nb, MT_T, 0, st>>>(pred, pred_stride, labels, n, part);
  bm_final<<<1, MT_T, 0, st>>>(part, nb, n, accumulate, static_cast<unsigned long long*>(result));
  return launch_status("rs_binary_metrics");
}

static bool auc_shape_ok(const char* what, int grouped, int64_t n_groups, int64_t n) {
  if (n < 0 || n >= MT_NMAX) {
    set_error("%s: need 0 <= n < 2^31", what);
    return false;
  }
  if (grouped && (n_groups < 1 || n_groups >= MT_NMAX)) {
    set_error("%s: need 1 <= n_groups < 2^31 with group ids", what);
    return false;
  }
  return true;
}

extern "C" int64_t rs_auc_workspace_size(int64_t n, int64_t n_groups) {
  if (!auc_shape_ok("rs_auc_workspace_size", n_groups != 0, n_groups, n)) return -1;
  return auc_ws(n, n_groups).total;
}

extern "C" int rs_auc(const float* scores, int64_t score_stride, const float* labels, const void* group_ids,
                      int group_kind, int64_t n_groups, int64_t n, void* result, void* workspace,
                      rs_stream_t stream) {
  const bool grouped = group_ids != nullptr;
  if (!auc_shape_ok("rs_auc", grouped, n_groups, n)) return RS_ERR_ARG;
  RS_REQUIRE(result && workspace, "rs_auc: null pointer");
  RS_REQUIRE(n == 0 || (scores && labels && score_stride >= 1), "rs_auc: null pointer or score_stride < 1");
  RS_REQUIRE(!grouped || group_kind == RS_ID_I32 || group_kind == RS_ID_I64,
             "rs_auc: group ids are int32 or int64 (RS_ID_I32 / RS_ID_I64)");
  hipStream_t st = as_stream(stream);
  const int64_t G = grouped ? n_groups : 0;
  const AucWs w = auc_ws(n, G);
  uint8_t* base = static_cast<uint8_t*>(workspace);
  auto u32 = [&](int64_t off) { return reinterpret_cast<uint32_t*>(base + off); };
  auto i32 = [&](int64_t off) { return reinterpret_cast<int32_t*>(base + off); };
  long long* cnt = reinterpret_cast<long long*>(base + w.cnt);
  long long* gu2 = reinterpret_cast<long long*>(base + w.gu2);
  unsigned long long* res = static_cast<unsigned long long*>(result);
  const int64_t ninit = G > AC_WORDS ? G : AC_WORDS;
  auc_init<<<(unsigned)((ninit + MT_T - 1) / MT_T), MT_T, 0, st>>>(cnt, gu2, i32(w.gstart), i32(w.gend), G);
  if (n == 0) {
    auc_final<<<1, 64, 0, st>>>(cnt, i32(w.cpos), n, res);
    return launch_status("rs_auc");
  }
  const unsigned nb = (unsigned)((n + MT_T - 1) / MT_T);
  auc_keys<<<nb, MT_T, 0, st>>>(scores, score_stride, labels, n, u32(w.key0), u32(w.a), cnt);
  (void)sort_pairs_u32(u32(w.key0), u32(w.a), u32(w.b), u32(w.idx1), n, 32, base + w.sort, st);
  auc_flags<false><<<nb, MT_T, 0, st>>>(u32(w.b), nullptr, u32(w.idx1), n, i32(w.cpos), i32(w.chead), nullptr, nullptr);
  (void)inclusive_sum_i32(i32(w.cpos), i32(w.cpos), n, base + w.scan, st);
  (void)inclusive_sum_i32(i32(w.chead), i32(w.chead), n, base + w.scan, st);
  auc_run_starts<<<nb, MT_T, 0, st>>>(i32(w.chead), n, i32(w.start));
  auc_runs<<<nb < MT_MAXB ? nb : MT_MAXB, MT_T, 0, st>>>(i32(w.cpos), i32(w.chead), i32(w.start), n, cnt);
  auc_final<<<1, 64, 0, st>>>(cnt, i32(w.cpos), n, res);
  if (grouped) {
    int bits = 1;
    while (bits < 32 && (1ll << bits) < G) ++bits;
    with_id_kind(group_kind, [&](auto kind) {
      if constexpr (decltype(kind)::value < 2)
        auc_group_keys<decltype(kind)::value><<<nb, MT_T, 0, st>>>(group_ids, G, u32(w.idx1), n, u32(w.a), cnt);
    });
    (void)sort_pairs_u32(u32(w.a), u32(w.idx1), u32(w.b), u32(w.idx2), n, bits, base + w.sort, st);
    auc_flags<true><<<nb, MT_T, 0, st>>>(u32(w.key0), u32(w.b), u32(w.idx2), n, i32(w.cpos), i32(w.chead),
                                         i32(w.gstart), i32(w.gend));
    (void)inclusive_sum_i32(i32(w.cpos), i32(w.cpos), n, base + w.scan, st);
    (void)inclusive_sum_i32(i32(w.chead), i32(w.chead), n, base + w.scan, st);
    auc_run_starts<<<nb, MT_T, 0, st>>>(i32(w.chead), n, i32(w.start));
    auc_group_runs<<<nb, MT_T, 0, st>>>(i32(w.cpos), i32(w.chead), i32(w.start), n, u32(w.b), i32(w.gstart), gu2);
    const int gb = gt_blocks(G);
    const int64_t chunk = (G + gb - 1) / gb;
    unsigned long long* gpart = reinterpret_cast<unsigned long long*>(base + w.gpart);
    auc_group_terms<<<gb, MT_T, 0, st>>>(gu2, i32(w.gstart), i32(w.gend), i32(w.cpos), G, chunk, gpart);
    auc_group_final<<<1, MT_T, 0, st>>>(gpart, gb, cnt, res);
  }
  return launch_status("rs_auc");
}
