// dssm.hip — the forward of DSSM (model/dssm.py), the reference's two-tower
// retrieval model: var-len pooling from ids, a whole tower in one launch, the
// row normalisation, and the in-batch sampled-softmax loss.
//
//   rs_seq_pool_fwd     SequencePoolingLayer (layer/sequence.py:20-95) from ids
//                       (or from embedded values): one WAVE per (sample,
//                       feature).  A row of E floats is read by E / 4 lanes
//                       (float4 each; E lanes when 4 does not divide E), so a
//                       wave holds G = min(64 / lanes-per-row, 16) rows at
//                       once: lane group g adds positions t = g, g + G, ... in
//                       ascending order, and the G partial rows are then added
//                       in group order (shuffles) — a fixed order per sample,
//                       independent of the batch.  The rows of masked positions
//                       are never loaded.
//   rs_dssm_tower_fwd   [SparseFeat rows | pooled var-len features | dense
//                       values] staged straight into the 16-sample LDS tile
//                       (wave r stages sample r; sequence pieces through the
//                       pooling function above), the DNN tower on the
//                       rs_mlp_prepare packing (mlp_tower_tile<NW, true>: its last
//                       layer kept in LDS), then l2_normalize of each row.
//   rs_l2_normalize_fwd the same row function as a launch of its own.
//   rs_inbatch_softmax_fwd  InBatchSoftmaxLayer (layer/activation.py:267-285,
//                       layer/utils.py:206-215): a workgroup owns 16 user rows
//                       (u / temperature, in LDS); its 16 waves walk the item
//                       column tiles (wave w: tiles w, w + 16, ...) with
//                       v_mfma_f32_16x16x4_f32 and keep a running (max, sum)
//                       per row and lane; the 16 lanes of a row merge in a
//                       fixed butterfly, the waves' partials in wave order.
//                       The [B, B] logits exist only in registers.
//   rs_dssm_score_fwd   the 'logistic' head: sigmoid(u . v / temperature).
#include "dssm_softmax.hpp"

namespace rs {

constexpr int SP_MAXF = 8;   // sequence features per launch
constexpr int SP_MAXG = 16;  // rows a wave holds at once
constexpr int SP_U = 8;      // positions per lane group in flight (one round covers T = 64 at E = 32)
constexpr int SP_MAXE = 256;
enum { POOL_SUM = 0, POOL_MEAN = 1, POOL_MAX = 2 };

struct SeqFeat {
  const void* src;            // ids [B, T] (src_stride apart) or values [B, T, E] (table == null)
  const float* table;         // [vocab, E]; null = a dense-values source
  const void* len;            // lengths [B] or null
  const unsigned char* mask;  // dense source without lengths: [B, T], non-zero = valid
  int64_t src_stride, vocab;
  int kind, len_kind, T, E, comb, out_col, v;  // v: floats per lane (4 or 1)
};
struct SeqPoolArgs {
  int nf;
  SeqFeat f[SP_MAXF];
  float* out;
  int64_t out_stride, batch;
  int* err;
};

// one id: validity (decode's), the clamped id, and whether the raw value is non-zero (Keras mask_zero)
__device__ __forceinline__ bool sp_id(int kind, const void* p, int64_t off, int64_t vocab, int64_t& id, bool& nz) {
  switch (kind) {
    case RS_ID_I32: {
      const auto r = Ids<0>::load(p, off);
      nz = r != 0;
      return Ids<0>::decode(r, vocab, id);
    }
    case RS_ID_I64: {
      const auto r = Ids<1>::load(p, off);
      nz = r != 0;
      return Ids<1>::decode(r, vocab, id);
    }
    default: {
      const auto r = Ids<2>::load(p, off);
      nz = r != 0.f;
      return Ids<2>::decode(r, vocab, id);
    }
  }
}

// The pooled row of feature f for sample b, computed by one whole wave: lane
// c < E / V receives columns V c .. V c + V - 1 in res (every lane group holds
// the same totals).  bad: an id out of range at a valid position.
template <int V>
__device__ __forceinline__ void seq_pool_row(const SeqFeat& f, int64_t b, float (&res)[V], bool& bad) {
  typedef typename VecF<V>::T vec_t;
  const int lane = threadIdx.x & 63;
  const int T = f.T, LPR = f.E / V;
  int G = 64 / LPR;
  if (G > SP_MAXG) G = SP_MAXG;
  const int g = lane / LPR, c = lane - g * LPR;
  const bool dense = f.table == nullptr, by_len = f.len != nullptr;
  const bool is_max = f.comb == POOL_MAX;

  int64_t len = 0;
  int nvalid;
  float flen;
  if (by_len) {
    len = f.len_kind == RS_ID_I64 ? static_cast<const int64_t*>(f.len)[b]
                                  : static_cast<int64_t>(static_cast<const int32_t*>(f.len)[b]);
    flen = static_cast<float>(len);
    nvalid = len <= 0 ? 0 : (len >= T ? T : static_cast<int>(len));
  } else {  // the mask's row sum (supports_masking=True): non-zero ids / mask bytes
    int cnt = 0;
    for (int t0 = 0; t0 < T; t0 += 64) {
      const int t = t0 + lane;
      bool nz = false;
      if (t < T) {
        if (dense) {
          nz = f.mask[b * T + t] != 0;
        } else {
          int64_t id;
          sp_id(f.kind, f.src, b * f.src_stride + t, f.vocab, id, nz);
        }
      }
      cnt += __popcll(__ballot(nz));
    }
    nvalid = cnt;
    flen = static_cast<float>(cnt);
  }

  float acc[V];
#pragma unroll
  for (int j = 0; j < V; ++j) acc[j] = is_max ? -INFINITY : 0.f;
  // A round = SP_U positions per lane group, in four stages, so that it costs
  // two memory trips: the ids of its positions (all of them: an id does not
  // wait for the length), their decode, the valid rows, the sums.
  auto rounds = [&](auto KC) {
    constexpr int K = decltype(KC)::value;  // 0 .. 2: ids of that kind; 3: a dense-values source
    typedef Ids<K == 3 ? 0 : K> I;
    for (int t0 = g; t0 < T; t0 += G * SP_U) {
      typename I::raw_t raw[SP_U];
      unsigned char mk[SP_U];
#pragma unroll
      for (int u = 0; u < SP_U; ++u) {
        const int t = min(t0 + u * G, T - 1);  // (in bounds; a position past T is dropped below)
        raw[u] = 0;
        mk[u] = 1;
        if constexpr (K == 3) {
          if (!by_len) mk[u] = f.mask[b * T + t];
        } else {
          raw[u] = I::load(f.src, b * f.src_stride + t);
        }
      }
      bool valid[SP_U], ok[SP_U];
      const float* rp[SP_U];
#pragma unroll
      for (int u = 0; u < SP_U; ++u) {
        const int t = t0 + u * G;
        if constexpr (K == 3) {
          ok[u] = true;
          valid[u] = t < T && (by_len ? t < len : mk[u] != 0);
          rp[u] = static_cast<const float*>(f.src) + b * f.src_stride + (int64_t)min(t, T - 1) * f.E + V * c;
        } else {
          int64_t id;
          ok[u] = I::decode(raw[u], f.vocab, id);
          valid[u] = t < T && (by_len ? t < len : raw[u] != 0);  // (Keras mask_zero: the raw id)
          rp[u] = f.table + id * f.E + V * c;
        }
      }
      vec_t r[SP_U];
#pragma unroll
      for (int u = 0; u < SP_U; ++u) {
        r[u] = vec_t{};
        if (valid[u] && ok[u]) r[u] = *reinterpret_cast<const vec_t*>(rp[u]);  // (a masked position is not loaded)
      }
#pragma unroll
      for (int u = 0; u < SP_U; ++u) {
        if (valid[u]) {
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const float x = VecF<V>::get(r[u], j);
            acc[j] = is_max ? fmaxf(acc[j], x) : acc[j] + x;
          }
          bad |= !ok[u];
        }
      }
    }
  };
  if (g < G) {
    if (dense) {
      rounds(std::integral_constant<int, 3>());
    } else {
      switch (f.kind) {
        case RS_ID_I32: rounds(std::integral_constant<int, 0>()); break;
        case RS_ID_I64: rounds(std::integral_constant<int, 1>()); break;
        default: rounds(std::integral_constant<int, 2>()); break;
      }
    }
  }
  // the lane groups' partial rows, in group order
#pragma unroll
  for (int j = 0; j < V; ++j) {
    float tot = __shfl(acc[j], c);
    for (int gg = 1; gg < G; ++gg) {
      const float p = __shfl(acc[j], gg * LPR + c);
      tot = is_max ? fmaxf(tot, p) : tot + p;
    }
    // max of x - (1 - mask) * 1e9: a masked position is -1e9 (exact while |x| < 32)
    if (is_max && nvalid < T) tot = fmaxf(tot, -1e9f);
    if (f.comb == POOL_MEAN) tot = tot / (flen + 1e-8f);
    res[j] = tot;
  }
}

// ... written to dst[V c + j] by the lanes of group 0 (dst: the feature's first column of a global or an LDS row)
__device__ __forceinline__ void seq_pool_store(const SeqFeat& f, int64_t b, float* dst, bool& bad) {
  const int lane = threadIdx.x & 63;
  if (f.v == 4) {
    float res[4];
    seq_pool_row<4>(f, b, res, bad);
    if (lane < f.E / 4) {
#pragma unroll
      for (int j = 0; j < 4; ++j) dst[4 * lane + j] = res[j];
    }
  } else {
    float res[1];
    seq_pool_row<1>(f, b, res, bad);
    if (lane < f.E) dst[lane] = res[0];
  }
}

__global__ __launch_bounds__(256) void seq_pool_kernel(SeqPoolArgs a) {
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t item = (int64_t)blockIdx.x * 4 + w;
  if (item >= a.batch * a.nf) return;
  const int64_t b = item / a.nf;
  const int fi = (int)(item - b * a.nf);
  const SeqFeat& f = a.f[fi];
  bool bad = false;
  seq_pool_store(f, b, a.out + b * a.out_stride + f.out_col, bad);
  if (__any(bad) && (threadIdx.x & 63) == 0) flag_error(a.err);
}

// tf.math.l2_normalize(axis=-1) of one row by one wave: x * rsqrt(max(sum x^2,
// 1e-12)); lane l adds columns l, l + 64, ... ascending (fma), then the fixed
// xor butterfly over the wave.  x: a global or an LDS row.
__device__ __forceinline__ void l2norm_row(const float* x, int N, float* y) {
  const int lane = threadIdx.x & 63;
  float s = 0.f;
  for (int c = lane; c < N; c += 64) s = fmaf(x[c], x[c], s);
  s = wave_sum(s);
  const float inv = rsqrtf(fmaxf(s, 1e-12f));
  for (int c = lane; c < N; c += 64) y[c] = x[c] * inv;
}

__global__ __launch_bounds__(256) void l2_normalize_kernel(const float* x, int64_t xs, float* y, int64_t ys, int64_t M,
                                                           int N) {
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t m = (int64_t)blockIdx.x * 4 + w;
  if (m >= M) return;
  l2norm_row(x + m * xs, N, y + m * ys);
}

// ---- one tower in one launch
struct DssmTowerArgs {
  float* out;
  int64_t out_stride;
  int n_out;  // the embedding's width (the last layer's, or the input's with no layer)
};

template <int NW>
__global__ __launch_bounds__(NW * 64) void dssm_tower_kernel(MlpArgs a, ConcatArgs pc, SeqPoolArgs sp,
                                                            DssmTowerArgs d) {
  extern __shared__ float smem[];
  const int RS = a.rs;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t m0 = (int64_t)blockIdx.x * 16;

  floatx4 ring[MLP_R];
  if (a.L > 0) mlp_first_fill<NW>(a, ring);
  // The input row of sample m0 + w (rows past M re-read row M - 1 and are
  // never stored).  Four columns per lane in flight, two memory trips: every
  // column's id, then its value.  A column finds its piece in a loop over the
  // pieces whose index is wave-uniform, so the descriptors come through scalar
  // loads and selects: indexing the kernel-argument arrays by a per-lane piece
  // number costs one dependent vector load per field.  The sequence pieces are
  // pooled first (their state and the columns' do not fit the registers together).
  const int Kp0 = a.L > 0 ? a.Kp[0] : (a.K0 + 15) & ~15;
  {
    const int r = w;
    const bool live = m0 + r < a.M;
    const int64_t m = live ? m0 + r : a.M - 1;
    bool bad = false;
    for (int fi = 0; fi < sp.nf; ++fi) seq_pool_store(sp.f[fi], m, smem + r * RS + sp.f[fi].out_col, bad);
    for (int c0 = 0; c0 < Kp0; c0 += 256) {
      int kind[4], j[4], wd[4];
      const void* src[4];
      const float* tab[4];
      int64_t voc[4];
      unsigned lo[4], hi[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int c = c0 + 64 * u + lane;
        kind[u] = -2;  // no piece: a sequence column, or padding past K0
        j[u] = wd[u] = 0;
        src[u] = nullptr;
        tab[u] = nullptr;
        voc[u] = 0;
        int64_t st = 0;
        for (int q = 0; q < pc.np; ++q) {
          const int oc = pc.out_col[q], wq = pc.col0[q + 1] - pc.col0[q];
          if (c >= oc && c < oc + wq) {
            kind[u] = pc.kind[q];
            j[u] = c - oc;
            wd[u] = wq;
            src[u] = pc.src[q];
            tab[u] = pc.table[q];
            voc[u] = pc.vocab[q];
            st = pc.src_stride[q];
          }
        }
        lo[u] = hi[u] = 0;
        if (kind[u] >= 0) {  // the id, as raw words (no wait here: decoded below)
          const char* ip = static_cast<const char*>(src[u]) + m * st * (kind[u] == RS_ID_I64 ? 8 : 4);
          lo[u] = *reinterpret_cast<const unsigned*>(ip);
          if (kind[u] == RS_ID_I64) hi[u] = *reinterpret_cast<const unsigned*>(ip + 4);
        } else if (kind[u] == -1) {
          src[u] = static_cast<const float*>(src[u]) + m * st + j[u];  // a dense value's address
        }
      }
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float* vp = nullptr;
        if (kind[u] >= 0) {
          int64_t id;
          bool ok;
          if (kind[u] == RS_ID_I64)
            ok = Ids<1>::decode(static_cast<int64_t>((static_cast<unsigned long long>(hi[u]) << 32) | lo[u]), voc[u], id);
          else if (kind[u] == RS_ID_F32) ok = Ids<2>::decode(__uint_as_float(lo[u]), voc[u], id);
          else ok = Ids<0>::decode(static_cast<int32_t>(lo[u]), voc[u], id);
          bad |= !ok;
          if (ok) vp = tab[u] + id * wd[u] + j[u];
        } else if (kind[u] == -1) {
          vp = static_cast<const float*>(src[u]);
        }
        v[u] = 0.f;
        if (vp) v[u] = *vp;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int c = c0 + 64 * u + lane;
        if (c < Kp0 && (kind[u] != -2 || c >= a.K0)) smem[r * RS + c] = v[u];  // (sequence columns: written above)
      }
    }
    if (__any(bad && live) && lane == 0) flag_error(pc.err);
  }
  int lastbuf = 0;
  if (a.L > 0) {
    float* par = smem + 32 * RS + NW * 256;
    for (int i = threadIdx.x; i < a.ptot; i += NW * 64) par[i] = a.prep[a.wtot + i];
    mlp_tower_tile<NW, true>(a, smem, m0, ring);
    lastbuf = a.L & 1;
  }
  __syncthreads();
  if (m0 + w < a.M)
    l2norm_row(smem + (lastbuf ? 16 * RS : 0) + w * RS, d.n_out, d.out + (m0 + w) * d.out_stride);
}

// ---- in-batch softmax (the tile walk: dssm_softmax.hpp, shared with the training forward)
__global__ __launch_bounds__(IB_NW * 64) void inbatch_softmax_kernel(IbsArgs a) { inbatch_softmax_tile<false>(a); }

__global__ __launch_bounds__(256) void dssm_score_kernel(const float* u, int64_t us, const float* v, int64_t vs,
                                                         float temp, float* out, int64_t B, int E) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t b = (int64_t)blockIdx.x * 4 + w;
  if (b >= B) return;
  float s = 0.f;
  for (int c = lane; c < E; c += 64) s = fmaf(u[b * us + c], v[b * vs + c], s);
  s = wave_sum(s);
  if (lane == 0) out[b] = sigmoidf_(s / temp);
}

// ---- host side
static int sp_fill(const char* what, int n_feat, const int* widths, const int* out_cols, const int* Ts,
                   const int* combiners, const int* kinds, const void* const* srcs, const int64_t* src_strides,
                   const float* const* tables, const int64_t* vocabs, const void* const* lengths,
                   const int* len_kinds, const void* const* masks, int64_t out_stride, SeqPoolArgs& a) {
  RS_REQUIRE(n_feat >= 1 && n_feat <= SP_MAXF, "%s: 1..%d sequence features", what, SP_MAXF);
  RS_REQUIRE(widths && out_cols && Ts && combiners && kinds && srcs && src_strides, "%s: null pointer", what);
  a.nf = n_feat;
  for (int i = 0; i < n_feat; ++i) {
    SeqFeat& f = a.f[i];
    const int E = widths[i], T = Ts[i];
    const bool dense = kinds[i] == -1;
    RS_REQUIRE(dense || (kinds[i] >= RS_ID_I32 && kinds[i] <= RS_ID_F32), "%s: feature %d: bad kind", what, i);
    RS_REQUIRE(E >= 1 && E <= SP_MAXE && (E % 4 == 0 || E <= 64),
               "%s: feature %d: width must be 1..64, or a multiple of 4 up to %d", what, i, SP_MAXE);
    RS_REQUIRE(T >= 1 && T <= (1 << 20), "%s: feature %d: bad T", what, i);
    RS_REQUIRE(combiners[i] >= POOL_SUM && combiners[i] <= POOL_MAX, "%s: feature %d: combiner must be 0 (sum), 1 (mean) or 2 (max)", what, i);
    RS_REQUIRE(srcs[i] && out_cols[i] >= 0 && (int64_t)out_cols[i] + E <= out_stride,
               "%s: feature %d: bad source / column", what, i);
    RS_REQUIRE(src_strides[i] >= (dense ? (int64_t)T * E : (int64_t)T), "%s: feature %d: bad source stride", what, i);
    RS_REQUIRE(dense || (tables && tables[i] && vocabs && vocabs[i] >= 1), "%s: feature %d needs a table and a vocab",
               what, i);
    f.len = lengths ? lengths[i] : nullptr;
    f.len_kind = RS_ID_I32;
    if (f.len) {
      RS_REQUIRE(len_kinds && (len_kinds[i] == RS_ID_I32 || len_kinds[i] == RS_ID_I64),
                 "%s: feature %d: lengths are int32 or int64", what, i);
      f.len_kind = len_kinds[i];
    }
    f.mask = (dense && !f.len && masks) ? static_cast<const unsigned char*>(masks[i]) : nullptr;
    RS_REQUIRE(!dense || f.len || f.mask, "%s: feature %d: a dense-values source needs lengths or a mask", what, i);
    f.src = srcs[i];
    f.table = dense ? nullptr : tables[i];
    f.src_stride = src_strides[i];
    f.vocab = dense ? 0 : vocabs[i];
    f.kind = kinds[i];
    f.T = T;
    f.E = E;
    f.comb = combiners[i];
    f.out_col = out_cols[i];
    // float4 rows need 16-byte row starts
    const void* base = dense ? srcs[i] : static_cast<const void*>(tables[i]);
    const bool v4 = E % 4 == 0 && (reinterpret_cast<uintptr_t>(base) & 15) == 0 && (!dense || src_strides[i] % 4 == 0);
    RS_REQUIRE(v4 || E <= 64, "%s: feature %d: rows wider than 64 need 16-byte alignment", what, i);
    f.v = v4 ? 4 : 1;
  }
  return RS_OK;
}

// LDS geometry of the one-launch tower (n_layers == 0: the staged tile alone)
static bool dssm_geom(int n_layers, const int* dims, MlpGeom& g) {
  if (!dims || n_layers < 0 || n_layers > MLP_MAXL) return false;
  if (n_layers > 0) return mlp_geom(n_layers, dims, g);
  if (dims[0] < 1 || dims[0] > MLP_MAXD) return false;
  g = MlpGeom{};
  g.rs = rup(rup(dims[0], 16), 64) + 8;
  g.lds = (size_t)16 * g.rs * sizeof(float);
  return true;
}

static bool dssm_tower_ok(int n_pieces, int n_layers, const int* dims, const int* acts, MlpGeom& g) {
  if (n_pieces < 1 || n_pieces > CC_MAXP || !dssm_geom(n_layers, dims, g)) return false;
  if (n_layers == 0) return true;
  if (!acts) return false;
  for (int l = 0; l < n_layers; ++l)
    if (acts[l] != RS_ACT_NONE && acts[l] != RS_ACT_RELU && acts[l] != RS_ACT_SIGMOID) return false;
  // rs_mlp_fwd runs these widths (a 256 -> 128 -> 64 -> 1 tail) as its split-K
  // tail, which sums in another order: not this kernel's tower
  int gwa = 0, gwb = 0;
  if (mlp_tail_ok(g.Np, g.Kp, g.N, g.L, 1, gwa, gwb) && gwa == 8 && gwb == 2) return false;
  return true;
}

}  // namespace rs

using namespace rs;

extern "C" int rs_seq_pool_fwd(int n_feat, const int* widths, const int* out_cols, const int* Ts,
                               const int* combiners, const int* kinds, const void* const* srcs,
                               const int64_t* src_strides, const float* const* tables, const int64_t* vocabs,
                               const void* const* lengths, const int* len_kinds, const void* const* masks, float* out,
                               int64_t out_stride, int64_t batch, int* err_flag, rs_stream_t stream) {
  RS_REQUIRE(batch >= 0, "rs_seq_pool_fwd: negative batch");
  SeqPoolArgs a{};
  const int st = sp_fill("rs_seq_pool_fwd", n_feat, widths, out_cols, Ts, combiners, kinds, srcs, src_strides, tables,
                         vocabs, lengths, len_kinds, masks, out_stride, a);
  if (st != RS_OK) return st;
  RS_REQUIRE(out, "rs_seq_pool_fwd: null output");
  if (batch == 0) return RS_OK;
  const int64_t grid = (batch * n_feat + 3) / 4;
  RS_REQUIRE(grid < (1ll << 31), "rs_seq_pool_fwd: batch too large");
  a.out = out;
  a.out_stride = out_stride;
  a.batch = batch;
  a.err = err_flag;
  seq_pool_kernel<<<(unsigned)grid, 256, 0, as_stream(stream)>>>(a);
  return launch_status("rs_seq_pool_fwd");
}

extern "C" int rs_l2_normalize_fwd(const float* x, int64_t x_stride, float* y, int64_t y_stride, int64_t M, int N,
                                   rs_stream_t stream) {
  RS_REQUIRE(M >= 0 && N >= 1 && x_stride >= N && y_stride >= N, "rs_l2_normalize_fwd: bad shape / stride");
  if (M == 0) return RS_OK;
  RS_REQUIRE(x && y, "rs_l2_normalize_fwd: null pointer");
  const int64_t grid = (M + 3) / 4;
  RS_REQUIRE(grid < (1ll << 31), "rs_l2_normalize_fwd: too many rows");
  l2_normalize_kernel<<<(unsigned)grid, 256, 0, as_stream(stream)>>>(x, x_stride, y, y_stride, M, N);
  return launch_status("rs_l2_normalize_fwd");
}

extern "C" int rs_dssm_tower_ok(int n_pieces, int n_layers, const int* dims, const int* acts) {
  MlpGeom g;
  return dssm_tower_ok(n_pieces, n_layers, dims, acts, g) ? 1 : 0;
}

extern "C" int rs_dssm_tower_fwd(int n_pieces, const int* widths, const int* in_cols, const int* kinds,
                                 const void* const* srcs, const int64_t* src_strides, const float* const* tables,
                                 const int64_t* vocabs, int n_seq, const int* seq_widths, const int* seq_cols,
                                 const int* seq_Ts, const int* combiners, const int* seq_kinds,
                                 const void* const* seq_srcs, const int64_t* seq_strides,
                                 const float* const* seq_tables, const int64_t* seq_vocabs,
                                 const void* const* lengths, const int* len_kinds, const void* const* masks,
                                 int n_layers, const int* dims, const int* acts, const float* prepared, float* out,
                                 int64_t out_stride, int64_t batch, int* err_flag, rs_stream_t stream) {
  const char* what = "rs_dssm_tower_fwd";
  RS_REQUIRE(batch >= 0 && n_pieces >= 0 && n_seq >= 0, "%s: negative count", what);
  MlpGeom g;
  RS_REQUIRE(dssm_tower_ok(n_pieces + n_seq, n_layers, dims, acts, g),
             "%s: shape not supported (rs_dssm_tower_ok: 1..%d pieces, 0..%d layers of widths 1..%d with none / relu / "
             "sigmoid, the tile's LDS <= 160 KiB, no split-K tail shape)",
             what, CC_MAXP, MLP_MAXL, MLP_MAXD);
  const int K0 = dims[0], n_out = dims[n_layers];
  ConcatArgs pc{};
  SeqPoolArgs sp{};
  if (n_pieces > 0) {
    const int st = concat_fill(n_pieces, widths, in_cols, kinds, srcs, src_strides, tables, vocabs, K0, what, pc);
    if (st != RS_OK) return st;
  }
  if (n_seq > 0) {
    const int st = sp_fill(what, n_seq, seq_widths, seq_cols, seq_Ts, combiners, seq_kinds, seq_srcs, seq_strides,
                           seq_tables, seq_vocabs, lengths, len_kinds, masks, K0, sp);
    if (st != RS_OK) return st;
  }
  // the pieces tile the input row exactly
  {
    unsigned char used[MLP_MAXD] = {};
    int cols = 0;
    auto mark = [&](int c0, int wd) {
      for (int c = c0; c < c0 + wd; ++c) {
        if (used[c]) return false;
        used[c] = 1;
      }
      cols += wd;
      return true;
    };
    for (int p = 0; p < n_pieces; ++p) RS_REQUIRE(mark(in_cols[p], widths[p]), "%s: pieces overlap", what);
    for (int p = 0; p < n_seq; ++p) RS_REQUIRE(mark(seq_cols[p], seq_widths[p]), "%s: pieces overlap", what);
    RS_REQUIRE(cols == K0, "%s: the pieces cover %d of the %d input columns", what, cols, K0);
  }
  RS_REQUIRE(out && out_stride >= n_out && err_flag, "%s: null / short output or null error flag", what);
  RS_REQUIRE(n_layers == 0 || prepared, "%s: null prepared weights", what);
  if (batch == 0) return RS_OK;
  MlpArgs a{};
  if (n_layers > 0) RS_REQUIRE(mlp_fill_args(g, acts, prepared, a), "%s: bad activation", what);
  a.L = n_layers;
  a.K0 = K0;
  a.rs = g.rs;
  a.M = batch;
  a.head = 0;
  pc.err = err_flag;
  pc.batch = batch;
  sp.batch = batch;
  DssmTowerArgs d{out, out_stride, n_out};
  const int64_t grid = (batch + 15) / 16;
  RS_REQUIRE(grid < (1ll << 31), "%s: batch too large", what);
  launch_lds<dssm_tower_kernel<MLP_NW>>((unsigned)grid, MLP_NW * 64, g.lds, as_stream(stream), a, pc, sp, d);
  return launch_status(what);
}

extern "C" int rs_inbatch_softmax_ok(int E) { return E >= 1 && E <= IB_MAXE ? 1 : 0; }

extern "C" int rs_inbatch_softmax_fwd(const float* user, int64_t user_stride, const float* item, int64_t item_stride,
                                      const void* item_idx, int idx_kind, const float* logq, int64_t n_items,
                                      float temperature, float* loss, int64_t batch, int E, int* err_flag,
                                      rs_stream_t stream) {
  const char* what = "rs_inbatch_softmax_fwd";
  IbsArgs a{};
  const int st = ib_fill(what, user, user_stride, item, item_stride, item_idx, idx_kind, logq, n_items, temperature,
                         loss, batch, E, err_flag, a);
  if (st != RS_OK || batch == 0) return st;
  inbatch_softmax_kernel<<<(unsigned)ib_grid(a), IB_NW * 64, ib_lds(a), as_stream(stream)>>>(a);
  return launch_status(what);
}

extern "C" int rs_dssm_score_fwd(const float* user, int64_t user_stride, const float* item, int64_t item_stride,
                                 float temperature, float* out, int64_t batch, int E, rs_stream_t stream) {
  const char* what = "rs_dssm_score_fwd";
  RS_REQUIRE(batch >= 0 && E >= 1 && user_stride >= E && item_stride >= E, "%s: bad shape / stride", what);
  RS_REQUIRE(temperature > 0.f, "%s: temperature must be positive", what);
  if (batch == 0) return RS_OK;
  RS_REQUIRE(user && item && out, "%s: null pointer", what);
  const int64_t grid = (batch + 3) / 4;
  RS_REQUIRE(grid < (1ll << 31), "%s: batch too large", what);
  dssm_score_kernel<<<(unsigned)grid, 256, 0, as_stream(stream)>>>(user, user_stride, item, item_stride, temperature,
                                                                  out, batch, E);
  return launch_status(what);
}
