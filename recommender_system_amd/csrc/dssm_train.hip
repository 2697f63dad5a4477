// dssm_train.hip — the training step of DSSM (model/dssm.py:149-152: Adam on
// the mean in-batch softmax loss):
//
//   rs_inbatch_softmax_train_fwd  rs_inbatch_softmax_fwd's tile walk
//                       (dssm_softmax.hpp) that also keeps lse[i] = logsumexp_j z_ij.
//   rs_inbatch_softmax_bwd  du and dv without a [B, B] buffer and without
//                       atomics, two launches of one kernel.  A workgroup OWNS
//                       16 rows of one side (users for du, items for dv) and
//                       its 8 waves walk the OTHER side's 16-row tiles (wave w:
//                       tiles w, w + 8, ...).  Per tile a wave stages the other
//                       rows X in its own LDS slab, recomputes the logits tile
//                       with v_mfma_f32_16x16x4_f32 as D[x][o] = sum_e X[x][e]
//                       O[o][e] — the OTHER index on the accumulator's rows
//                       (lane l holds rows 4 (l >> 4) + r, column l & 15) —
//                       forms dz in those registers, and feeds them straight
//                       back as the B operand of the second product
//                       acc[e][o] += sum_x X[x][e] dz[x][o]: an accumulator's
//                       row index (l >> 4, r) is exactly a B operand's k index
//                       (k slot l >> 4 of MFMA r), so no shuffle and no LDS
//                       round trip sits between the two products.  That fixes
//                       which product is computed transposed: du recomputes
//                       z^T (A = item rows, B = u / temperature), dv recomputes
//                       z (A = u / temperature, B = item rows).  The waves'
//                       partial [E][16] tiles are added in wave order.
//   rs_l2_normalize_bwd one wave per row, the forward's sums.
//   rs_embedding_grad_accum  dense G[id] += scale_b grad[b] over the valid
//                       positions of ids [B, T]: stable radix sort by row,
//                       segment sums in lookup order (seg_piece / seg_cross).
//   rs_adam_update_multi  Keras optimizer_v2 Adam over up to 32 tensors a
//                       launch, the step counter read from device memory;
//   rs_adam_advance     the counter's + 1, on the stream.
#include <cmath>

#include "dssm_softmax.hpp"
#include "radix_sort.hpp"

namespace rs {

__global__ __launch_bounds__(IB_NW * 64) void inbatch_softmax_train_kernel(IbsArgs a) {
  inbatch_softmax_tile<true>(a);
}

// ---- in-batch softmax backward
constexpr int IBB_NW = 8;
constexpr int IBB_MAXE = 256;  // 16 + 8 * 16 rows of E + 4 floats: 149,760 B of the 160 KiB at E = 256

struct IbbArgs {
  const float* user;
  int64_t us;
  const float* item;
  int64_t is;
  const void* idx;
  int idx_kind;
  const float* logq;
  int64_t n_items;
  float temp;
  const float* lse;
  const float* g;  // [B] or null = 1 / B
  float* out;      // du (DU) or dv
  int64_t os, B;
  int E, rs;
  int* err;
};

// DU: own = users (out = du = acc / temperature), other = items; else own =
// items (out = dv), other = users.  KGT: k-groups of 16 columns the
// accumulators are sized for (E <= 16 KGT).
template <bool DU, int KGT>
__global__ __launch_bounds__(IBB_NW * 64) void inbatch_softmax_bwd_kernel(IbbArgs a) {
  extern __shared__ float smem[];
  const int RS = a.rs;
  float* Os = smem;                                   // [16][RS] the own rows
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* Xs = smem + 16 * RS + w * 16 * RS;           // [16][RS] this wave's other rows
  float* rowv = smem + (IBB_NW + 1) * 16 * RS + w * 32;  // [16][2] per other row: (lq) or (lse, g)
  const int64_t o0 = (int64_t)blockIdx.x * 16;
  const int KG = (a.E + 15) >> 4, W = 16 * KG;
  const float inv_t = 1.0f / a.temp;
  const float gdef = 1.0f / (float)a.B;
  const float* own = DU ? a.user : a.item;
  const float* oth = DU ? a.item : a.user;
  const int64_t owns = DU ? a.us : a.is, oths = DU ? a.is : a.us;

  // own rows (u / temperature for DU), zero past B and past E
  for (int c = threadIdx.x; c < 16 * W; c += IBB_NW * 64) {
    const int r = c / W, e = c - r * W;
    float v = 0.f;
    if (o0 + r < a.B && e < a.E) {
      v = own[(o0 + r) * owns + e];
      if (DU) v = v / a.temp;
    }
    Os[r * RS + e] = v;
  }
  // this lane's own column o = lane & 15: (lse, g) for DU, log Q otherwise
  bool bad = false;
  float c_lse = 0.f, c_g = 0.f, c_lq = 0.f;
  {
    const int64_t o = o0 + (lane & 15);
    if (o < a.B) {
      if (DU) {
        c_lse = a.lse[o];
        c_g = a.g ? a.g[o] : gdef;
      } else {
        int64_t id;
        const bool ok = a.idx_kind == RS_ID_I64 ? cc_id<1>(a.idx, o, a.n_items, id) : cc_id<0>(a.idx, o, a.n_items, id);
        c_lq = ok ? a.logq[id] : 0.f;
        bad |= !ok && !DU && w == 0 && lane < 16;  // (flagged once, by the dv launch)
      }
    }
  }
  __syncthreads();

  floatx4 acc[KGT];
#pragma unroll
  for (int t = 0; t < KGT; ++t) acc[t] = floatx4{0.f, 0.f, 0.f, 0.f};
  const int64_t NT = (a.B + 15) >> 4;
  const float* ap = Xs + (lane & 15) * RS + 4 * (lane >> 4);
  const float* bp = Os + (lane & 15) * RS + 4 * (lane >> 4);
  for (int64_t xt = w; xt < NT; xt += IBB_NW) {
    const int64_t x0 = xt * 16;
    // stage the other rows (u / temperature when they are users), zero past B and past E
    for (int c = lane; c < 16 * W; c += 64) {
      const int r = c / W, e = c - r * W;
      float v = 0.f;
      if (x0 + r < a.B && e < a.E) {
        v = oth[(x0 + r) * oths + e];
        if (!DU) v = v / a.temp;
      }
      Xs[r * RS + e] = v;
    }
    if (lane < 16) {
      const int64_t x = x0 + lane;
      float v0 = 0.f, v1 = 0.f;
      if (x < a.B) {
        if (DU) {
          int64_t id;
          const bool ok =
              a.idx_kind == RS_ID_I64 ? cc_id<1>(a.idx, x, a.n_items, id) : cc_id<0>(a.idx, x, a.n_items, id);
          v0 = ok ? a.logq[id] : 0.f;
        } else {
          v0 = a.lse[x];
          v1 = a.g ? a.g[x] : gdef;
        }
      }
      rowv[2 * lane] = v0;
      rowv[2 * lane + 1] = v1;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // logits tile D[x][o]
    MacAcc<4> z;
    for (int q = 0; q < KG; ++q) {
      const floatx4 av = *reinterpret_cast<const floatx4*>(ap + 16 * q);
      const floatx4 bv = *reinterpret_cast<const floatx4*>(bp + 16 * q);
      z.mac4(av, bv);
    }
    const floatx4 dot = z.sum();
    float dz[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int xr = 4 * (lane >> 4) + r;
      const float lq = DU ? rowv[2 * xr] : c_lq;
      const float lse = DU ? c_lse : rowv[2 * xr];
      const float g = DU ? c_g : rowv[2 * xr + 1];
      const float p = expf((dot[r] - lq) - lse);
      const bool same = xt == blockIdx.x && xr == (lane & 15);
      dz[r] = x0 + xr < a.B ? g * (p - (same ? 1.0f : 0.0f)) : 0.f;
    }
    // acc[e][o] += sum_x X[x][e] dz[x][o]: MFMA r contracts x = 4 (l >> 4) + r
#pragma unroll
    for (int t = 0; t < KGT; ++t) {
      if (t < KG) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          acc[t] = mfma16x16x4(Xs[(4 * (lane >> 4) + r) * RS + 16 * t + (lane & 15)], dz[r], acc[t]);
      }
    }
    __builtin_amdgcn_wave_barrier();  // (the next tile's staging writes follow these reads in program order)
  }
  if (__any(bad) && lane == 0) flag_error(a.err);
  // the waves' partial tiles, added in wave order: the slabs become part[w][o][W]
  __syncthreads();
#pragma unroll
  for (int t = 0; t < KGT; ++t)
    if (t < KG) *reinterpret_cast<floatx4*>(Xs + (lane & 15) * RS + 16 * t + 4 * (lane >> 4)) = acc[t];
  __syncthreads();
  for (int c = threadIdx.x; c < 16 * W; c += IBB_NW * 64) {
    const int o = c / W, e = c - o * W;
    if (o0 + o < a.B && e < a.E) {
      float s = smem[16 * RS + o * RS + e];
      for (int p = 1; p < IBB_NW; ++p) s += smem[16 * RS + p * 16 * RS + o * RS + e];
      a.out[(o0 + o) * a.os + e] = DU ? s * inv_t : s;
    }
  }
}

// ---- l2_normalize backward: y = x r, r = rsqrt(max(s, 1e-12)); dx = r (dy - y (y . dy)), r dy below the floor
__global__ __launch_bounds__(256) void l2_normalize_bwd_kernel(const float* x, int64_t xs, const float* dy,
                                                               int64_t dys, float* dx, int64_t dxs, int64_t M, int N) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t m = (int64_t)blockIdx.x * 4 + w;
  if (m >= M) return;
  const float* xr = x + m * xs;
  const float* gr = dy + m * dys;
  float s = 0.f;
  for (int c = lane; c < N; c += 64) s = fmaf(xr[c], xr[c], s);
  s = wave_sum(s);
  const float inv = rsqrtf(fmaxf(s, 1e-12f));
  float d = 0.f;
  if (s >= 1e-12f) {
    for (int c = lane; c < N; c += 64) d = fmaf(xr[c] * inv, gr[c], d);
    d = wave_sum(d);
  }
  for (int c = lane; c < N; c += 64) dx[m * dxs + c] = inv * (gr[c] - (xr[c] * inv) * d);
}

// ---- dense table gradient from ids
enum { EGA_NONE = -1, EGA_SUM = 0, EGA_MEAN = 1 };

__device__ __forceinline__ int64_t ega_len(const void* len, int len_kind, int64_t b) {
  return len_kind == RS_ID_I64 ? static_cast<const int64_t*>(len)[b]
                               : static_cast<int64_t>(static_cast<const int32_t*>(len)[b]);
}

// scale[b] = 1 / (float(len_b) + 1e-8): len_b the length input, or the count of non-zero ids
template <int KIND>
__global__ __launch_bounds__(256) void ega_scale_kernel(const void* ids, int64_t id_stride, int T, const void* len,
                                                        int len_kind, int64_t B, float* __restrict__ scale) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  float flen;
  if (len) {
    flen = static_cast<float>(ega_len(len, len_kind, b));
  } else {
    int cnt = 0;
    for (int t = 0; t < T; ++t) cnt += Ids<KIND>::load(ids, b * id_stride + t) != 0;
    flen = static_cast<float>(cnt);
  }
  scale[b] = 1.0f / (flen + 1e-8f);
}

// key = the table row of a valid position (masked positions and bad ids: 0xffffffff, skipped), val = b T + t
template <int KIND>
__global__ __launch_bounds__(256) void ega_keys_kernel(const void* ids, int64_t id_stride, int T, const void* len,
                                                       int len_kind, int combiner, int64_t vocab, int64_t B,
                                                       uint32_t* __restrict__ key, uint32_t* __restrict__ val,
                                                       int* err) {
  typedef Ids<KIND> I;
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= B * T) return;
  const int64_t b = j / T;
  const int t = (int)(j - b * T);
  const typename I::raw_t raw = I::load(ids, b * id_stride + t);
  bool valid = true;
  if (combiner != EGA_NONE) valid = len ? (int64_t)t < ega_len(len, len_kind, b) : raw != 0;
  int64_t id;
  const bool ok = I::decode(raw, vocab, id);
  if (valid && !ok) flag_error(err);
  key[j] = valid && ok ? (uint32_t)id : 0xffffffffu;
  val[j] = (uint32_t)j;
}

__global__ __launch_bounds__(256) void ega_piece_kernel(const uint32_t* __restrict__ key,
                                                        const uint32_t* __restrict__ val, int64_t n, int T, int k,
                                                        const float* __restrict__ grad, int64_t ldg,
                                                        const float* __restrict__ scale, int64_t C,
                                                        float* __restrict__ part_first, float* __restrict__ part_last,
                                                        float* __restrict__ G) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t p = t / k;
  const int f = (int)(t - p * k);
  if (p >= n) return;
  uint32_t r;
  float s;
  if (seg_piece<32>(key, n, C, p, k, f, [&](int64_t q) {
        const uint32_t b = val[q] / (uint32_t)T;  // the gradient row is read through the sorted position
        const float v = grad[(int64_t)b * ldg + f];
        return scale ? scale[b] * v : v;
      }, part_first, part_last, r, s))
    G[(int64_t)r * k + f] += s;
}

__global__ __launch_bounds__(256) void ega_cross_kernel(const uint32_t* __restrict__ key, int64_t n, int k, int64_t C,
                                                        const float* __restrict__ part_first,
                                                        const float* __restrict__ part_last, float* __restrict__ G) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t p = t / k;
  const int f = (int)(t - p * k);
  if (p >= n) return;
  uint32_t r;
  float s;
  if (seg_cross(key, n, C, p, k, f, part_first, part_last, r, s)) G[(int64_t)r * k + f] += s;
}

// ---- Adam
constexpr int ADAM_MT = 32;
struct AdamMulti {
  float* w[ADAM_MT];
  const float* g[ADAM_MT];
  float* m[ADAM_MT];
  float* v[ADAM_MT];
  int64_t n[ADAM_MT];
  float l2[ADAM_MT];
  int first[ADAM_MT + 1];
  int count;
  float lr, b1, b2, omb1, omb2, lnb1, lnb2, eps;  // omb = 1 - beta and lnb = log(beta), computed in double
  const int64_t* step;
};

// tensor j owns blocks [first[j], first[j + 1]) of 1024 elements (4 per thread), as sgd_multi_kernel
__global__ __launch_bounds__(256) void adam_multi_kernel(const AdamMulti a) {
  const int blk = blockIdx.x;
  int j = 0;
  while (j + 1 < a.count && blk >= a.first[j + 1]) ++j;  // uniform, <= 32 steps
  float* __restrict__ w = a.w[j];
  const float* __restrict__ g = a.g[j];
  float* __restrict__ m = a.m[j];
  float* __restrict__ v = a.v[j];
  // lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t), 1 - beta^t = -expm1(t log beta): no cancellation at small t
  const float t = static_cast<float>(a.step[0] + 1);
  const float lr_t = a.lr * sqrtf(-expm1f(t * a.lnb2)) / -expm1f(t * a.lnb1);
  const float l2 = a.l2[j];
  const int64_t base = (int64_t)(blk - a.first[j]) * 1024 + threadIdx.x;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t i = base + 256 * u;
    if (i < a.n[j]) {
      const float wi = w[i];
      const float gi = g[i] + 2.f * l2 * wi;
      const float mi = a.b1 * m[i] + a.omb1 * gi;
      const float vi = a.b2 * v[i] + a.omb2 * (gi * gi);
      m[i] = mi;
      v[i] = vi;
      w[i] = wi - lr_t * mi / (sqrtf(vi) + a.eps);
    }
  }
}

__global__ void adam_advance_kernel(int64_t* step) {
  if (threadIdx.x == 0 && blockIdx.x == 0) step[0] += 1;
}

}  // namespace rs

using namespace rs;

extern "C" int rs_inbatch_softmax_train_fwd(const float* user, int64_t user_stride, const float* item,
                                            int64_t item_stride, const void* item_idx, int idx_kind,
                                            const float* logq, int64_t n_items, float temperature, float* loss,
                                            float* lse, int64_t batch, int E, int* err_flag, rs_stream_t stream) {
  const char* what = "rs_inbatch_softmax_train_fwd";
  IbsArgs a{};
  const int st = ib_fill(what, user, user_stride, item, item_stride, item_idx, idx_kind, logq, n_items, temperature,
                         loss, batch, E, err_flag, a);
  if (st != RS_OK || batch == 0) return st;
  RS_REQUIRE(lse, "%s: null pointer", what);
  a.lse = lse;
  inbatch_softmax_train_kernel<<<(unsigned)ib_grid(a), IB_NW * 64, ib_lds(a), as_stream(stream)>>>(a);
  return launch_status(what);
}

extern "C" int rs_inbatch_softmax_bwd_ok(int E) { return E >= 1 && E <= IBB_MAXE ? 1 : 0; }

template <bool DU>
static void ibb_launch(const IbbArgs& a, unsigned grid, size_t lds, hipStream_t st) {
  const int KG = (a.E + 15) / 16;
  if (KG <= 2) launch_lds<inbatch_softmax_bwd_kernel<DU, 2>>(grid, IBB_NW * 64, lds, st, a);
  else if (KG <= 4) launch_lds<inbatch_softmax_bwd_kernel<DU, 4>>(grid, IBB_NW * 64, lds, st, a);
  else if (KG <= 8) launch_lds<inbatch_softmax_bwd_kernel<DU, 8>>(grid, IBB_NW * 64, lds, st, a);
  else launch_lds<inbatch_softmax_bwd_kernel<DU, 16>>(grid, IBB_NW * 64, lds, st, a);
}

extern "C" int rs_inbatch_softmax_bwd(const float* user, int64_t user_stride, const float* item, int64_t item_stride,
                                      const void* item_idx, int idx_kind, const float* logq, int64_t n_items,
                                      float temperature, const float* lse, const float* g, float* du,
                                      int64_t du_stride, float* dv, int64_t dv_stride, int64_t batch, int E,
                                      int* err_flag, rs_stream_t stream) {
  const char* what = "rs_inbatch_softmax_bwd";
  RS_REQUIRE(batch >= 0, "%s: negative batch", what);
  RS_REQUIRE(rs_inbatch_softmax_bwd_ok(E), "%s: E must be 1..%d", what, IBB_MAXE);
  RS_REQUIRE(user_stride >= E && item_stride >= E && du_stride >= E && dv_stride >= E && n_items >= 1,
             "%s: bad stride / n_items", what);
  RS_REQUIRE(idx_kind == RS_ID_I32 || idx_kind == RS_ID_I64, "%s: item_idx is int32 or int64", what);
  RS_REQUIRE(temperature > 0.f, "%s: temperature must be positive", what);
  if (batch == 0) return RS_OK;
  RS_REQUIRE(user && item && item_idx && logq && lse && du && dv, "%s: null pointer", what);
  const int64_t grid = (batch + 15) / 16;
  RS_REQUIRE(grid < (1ll << 31), "%s: batch too large", what);
  IbbArgs a{};
  a.user = user;
  a.us = user_stride;
  a.item = item;
  a.is = item_stride;
  a.idx = item_idx;
  a.idx_kind = idx_kind;
  a.logq = logq;
  a.n_items = n_items;
  a.temp = temperature;
  a.lse = lse;
  a.g = g;
  a.B = batch;
  a.E = E;
  a.rs = (E + 15) / 16 * 16 + 4;
  a.err = err_flag;
  const size_t lds = ((size_t)(IBB_NW + 1) * 16 * a.rs + IBB_NW * 32) * sizeof(float);
  hipStream_t st = as_stream(stream);
  a.out = du;
  a.os = du_stride;
  ibb_launch<true>(a, (unsigned)grid, lds, st);
  a.out = dv;
  a.os = dv_stride;
  ibb_launch<false>(a, (unsigned)grid, lds, st);
  return launch_status(what);
}

extern "C" int rs_l2_normalize_bwd(const float* x, int64_t x_stride, const float* dy, int64_t dy_stride, float* dx,
                                   int64_t dx_stride, int64_t M, int N, rs_stream_t stream) {
  RS_REQUIRE(M >= 0 && N >= 1 && x_stride >= N && dy_stride >= N && dx_stride >= N,
             "rs_l2_normalize_bwd: bad shape / stride");
  if (M == 0) return RS_OK;
  RS_REQUIRE(x && dy && dx, "rs_l2_normalize_bwd: null pointer");
  const int64_t grid = (M + 3) / 4;
  RS_REQUIRE(grid < (1ll << 31), "rs_l2_normalize_bwd: too many rows");
  l2_normalize_bwd_kernel<<<(unsigned)grid, 256, 0, as_stream(stream)>>>(x, x_stride, dy, dy_stride, dx, dx_stride, M,
                                                                        N);
  return launch_status("rs_l2_normalize_bwd");
}

static int64_t ega_slab(int64_t n) { return (n * 4 + 255) / 256 * 256; }

extern "C" int64_t rs_embedding_grad_accum_workspace_size(int64_t n_lookups) {
  if (n_lookups < 0) return -1;
  return 6 * ega_slab(n_lookups) + (sort_pairs_ws_bytes(n_lookups) + 255) / 256 * 256;
}

extern "C" int rs_embedding_grad_accum(float* G, int64_t n_rows, int k, const void* ids, int id_kind,
                                       int64_t id_stride, int T, const void* lengths, int len_kind, int combiner,
                                       const float* grad, int64_t grad_stride, int64_t batch, void* workspace,
                                       int* err_flag, rs_stream_t stream) {
  const char* what = "rs_embedding_grad_accum";
  RS_REQUIRE(batch >= 0 && T >= 1 && T <= (1 << 20) && k >= 1 && n_rows >= 1, "%s: bad shape", what);
  RS_REQUIRE(id_kind >= RS_ID_I32 && id_kind <= RS_ID_F32, "%s: bad id_kind", what);
  RS_REQUIRE(combiner >= EGA_NONE && combiner <= EGA_MEAN, "%s: combiner must be -1 (none), 0 (sum) or 1 (mean)",
             what);
  RS_REQUIRE(combiner != EGA_NONE || !lengths, "%s: combiner -1 takes no lengths", what);
  RS_REQUIRE(!lengths || len_kind == RS_ID_I32 || len_kind == RS_ID_I64, "%s: lengths are int32 or int64", what);
  RS_REQUIRE(id_stride >= T && grad_stride >= k, "%s: bad stride", what);
  const int64_t n = batch * T;
  RS_REQUIRE(n_rows < 0xffffffffll && n < (1ll << 31) && n * k < (1ll << 38),
             "%s: rows must fit uint32, lookups int32", what);
  if (n == 0) return RS_OK;
  RS_REQUIRE(G && ids && grad && workspace, "%s: null pointer", what);
  const int64_t slab = ega_slab(n);
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  uint32_t* key_in = reinterpret_cast<uint32_t*>(ws);
  uint32_t* key_out = reinterpret_cast<uint32_t*>(ws + slab);
  uint32_t* val_in = reinterpret_cast<uint32_t*>(ws + 2 * slab);
  uint32_t* val_out = reinterpret_cast<uint32_t*>(ws + 3 * slab);
  float* part_first = reinterpret_cast<float*>(ws + 4 * slab);
  float* scale = combiner == EGA_MEAN ? reinterpret_cast<float*>(ws + 5 * slab) : nullptr;
  hipStream_t st = as_stream(stream);
  with_id_kind(id_kind, [&](auto K) {
    if (scale)
      ega_scale_kernel<decltype(K)::value><<<(unsigned)((batch + 255) / 256), 256, 0, st>>>(ids, id_stride, T, lengths,
                                                                                           len_kind, batch, scale);
    ega_keys_kernel<decltype(K)::value><<<(unsigned)((n + 255) / 256), 256, 0, st>>>(
        ids, id_stride, T, lengths, len_kind, combiner, n_rows, batch, key_in, val_in, err_flag);
  });
  // 2^bits > n_rows: the skip key 0xffffffff keeps its low bits all set, so it sorts after every row
  int bits = 1;
  while (bits < 32 && ((uint64_t)1 << bits) <= (uint64_t)n_rows) ++bits;
  const hipError_t e = sort_pairs_u32(key_in, val_in, key_out, val_out, n, bits, ws + 6 * slab, st);
  if (e != hipSuccess) {
    set_error("%s: radix sort failed: %s", what, hipGetErrorString(e));
    return RS_ERR_HIP;
  }
  const int64_t C = seg_chunk(k);
  const int64_t nchunk = (n + C - 1) / C;
  float* part_last = part_first + nchunk * k;
  const unsigned grid = (unsigned)((n * k + 255) / 256);
  ega_piece_kernel<<<grid, 256, 0, st>>>(key_out, val_out, n, T, k, grad, grad_stride, scale, C, part_first, part_last,
                                         G);
  if (nchunk > 1) ega_cross_kernel<<<grid, 256, 0, st>>>(key_out, n, k, C, part_first, part_last, G);
  return launch_status(what);
}

extern "C" int rs_adam_update_multi(int count, float* const* w, const float* const* grad, float* const* m,
                                    float* const* v, const int64_t* n, const float* l2, float lr, float beta1,
                                    float beta2, float eps, const int64_t* step, rs_stream_t stream) {
  const char* what = "rs_adam_update_multi";
  if (count == 0) return RS_OK;
  RS_REQUIRE(count > 0 && w && grad && m && v && n && l2 && step, "%s: bad arguments", what);
  RS_REQUIRE(lr >= 0 && beta1 > 0 && beta1 < 1 && beta2 > 0 && beta2 < 1 && eps >= 0,
             "%s: lr, eps >= 0 and 0 < beta < 1", what);
  for (int j = 0; j < count; ++j)
    RS_REQUIRE(w[j] && grad[j] && m[j] && v[j] && n[j] >= 0 && n[j] < (1ll << 40), "%s: bad tensor %d", what, j);
  hipStream_t st = as_stream(stream);
  for (int j0 = 0; j0 < count;) {
    AdamMulti a{};
    a.lr = lr;
    a.b1 = beta1;
    a.b2 = beta2;
    a.omb1 = (float)(1.0 - (double)beta1);  // of the float32 beta the caller holds, as Keras' float32 variables
    a.omb2 = (float)(1.0 - (double)beta2);
    a.lnb1 = (float)log((double)beta1);
    a.lnb2 = (float)log((double)beta2);
    a.eps = eps;
    a.step = step;
    int64_t blocks = 0;
    // pack tensors while the grid stays below 2^30 blocks (a tensor beyond that goes alone)
    while (j0 < count && a.count < ADAM_MT) {
      const int64_t nb = (n[j0] + 1023) / 1024;
      if (a.count > 0 && blocks + nb > (1ll << 30)) break;
      if (nb > 0) {
        a.w[a.count] = w[j0];
        a.g[a.count] = grad[j0];
        a.m[a.count] = m[j0];
        a.v[a.count] = v[j0];
        a.n[a.count] = n[j0];
        a.l2[a.count] = l2[j0];
        a.first[a.count] = (int)blocks;
        blocks += nb;
        ++a.count;
      }
      ++j0;
    }
    if (a.count == 0) continue;
    a.first[a.count] = (int)blocks;
    adam_multi_kernel<<<(unsigned)blocks, 256, 0, st>>>(a);
  }
  return launch_status(what);
}

extern "C" int rs_adam_advance(int64_t* step, rs_stream_t stream) {
  RS_REQUIRE(step, "rs_adam_advance: null pointer");
  adam_advance_kernel<<<1, 64, 0, as_stream(stream)>>>(step);
  return launch_status("rs_adam_advance");
}
