// afm_train.hip — the forward AND the row gradients of one AFM training step
// in one launch (rs_afm_train_fwd): ids -> rows -> pooled pairs -> Dense(1)
// -> sigmoid(s) -> BCE gradient -> dL/d(row) of every looked-up row, while
// the rows sit in registers.  The [B, P, k] pair tensor is never formed.
//
// Reference semantics (layer/interaction.py:322-351, model/afm.py:15-18,
// utils/compile_fit.py:9-15), e_f the row of field f, P = F(F-1)/2:
//   x_c  = pool over pairs (i<j) of e_ic e_jc   'att' sum / 'avg' sum/P / 'max'
//   z = x.w + b, s = sigmoid(z), p = sigmoid(s)
//   u = the input of the LAST sigmoid (Keras takes it as the BCE logit):
//       u = s with two sigmoids (AFM), u = z with one (AFMLayer)
//   loss = max(u,0) - u t + log1p(exp(-|u|)),  dL/du = (sigmoid(u) - t) / B
//   g = dL/dz = dL/du              (one sigmoid)
//             = dL/du s (1 - s)    (two)
//   dx_c = g w_c, S_c = sum_f e_fc
//   'att': de_fc = dx_c (S_c - e_fc);  'avg': the same / P
//   'max': (i*, j*) the arg-max pair of (b, c): de_{i*}c = dx_c e_{j*}c,
//          de_{j*}c = dx_c e_{i*}c, 0 for every other field.  Ties go to the
//          FIRST pair in row-major order (TF splits the gradient evenly among
//          tied pairs: documented deviation).
//   F = 1: no pair, x = 0 and de = 0; g is still produced (the bias trains).
// An out-of-range id reads the zero row (as the forward), sets the flag, and
// its own gradient block is 0.  No atomics: every output element has one
// writer, so two runs are bit-identical.
#include "rs_common.hpp"

namespace rs {

constexpr int TMAXF = 32;  // fields held in registers (rs_embed_pair_pool_fwd's PMAXF)

struct AfmTrainArgs {
  const void* ids;
  int64_t id_stride;
  const float* table;
  const int64_t* offs;
  const int64_t* vocab;
  int F, k;
  int mode;  // 0 sum ('att'), 1 mean over pairs, 2 max over pairs
  const float* head_w;
  const float* head_b;
  int n_sig;
  const float* labels;
  int64_t batch;
  float* pooled;
  int64_t pooled_stride;
  float* prob;  // optional
  float* g;
  float* loss;  // optional
  float* drows;
  int64_t drows_stride;
  bool vec_out;  // pooled and drows take float4 stores (16-byte aligned, strides % 4 == 0)
  int* err;
};

// The head from the logit z: writes prob / g / loss of sample b and returns g.
__device__ __forceinline__ float afm_head(const AfmTrainArgs& a, float z, int64_t b, bool write) {
  const float t = a.labels[b];
  const float s = sigmoidf_(z);
  float u = z, pu = s, dz = 1.f;
  if (a.n_sig == 2) {
    // s (1 - s) = e / (1 + e)^2 with e = exp(-|z|): no 1 - s cancellation where s saturates
    const float e = expf(-fabsf(z));
    dz = e / ((1.f + e) * (1.f + e));
    u = s;
    pu = sigmoidf_(s);
  }
  const float g = (pu - t) / (float)a.batch * dz;
  if (write) {
    if (a.prob) a.prob[b] = pu;
    a.g[b] = g;
    if (a.loss) a.loss[b] = fmaxf(u, 0.f) - u * t + log1pf(expf(-fabsf(u)));
  }
  return g;
}

template <int VW>
__device__ __forceinline__ void load_row(const float* p, float (&v)[VW]) {
  if constexpr (VW == 4) {
    const floatx4 t = __builtin_nontemporal_load(reinterpret_cast<const floatx4*>(p));
    v[0] = t[0], v[1] = t[1], v[2] = t[2], v[3] = t[3];
  } else {
    v[0] = *p;
  }
}
template <int VW>
__device__ __forceinline__ void store_row(float* p, const float (&v)[VW], bool vec) {
  if constexpr (VW == 4) {
    if (vec) {
      *reinterpret_cast<floatx4*>(p) = floatx4{v[0], v[1], v[2], v[3]};
      return;
    }
  }
#pragma unroll
  for (int t = 0; t < VW; ++t) p[t] = v[t];
}

// The lane layouts of pair_pool_kernel (interact.hip): VW = 4: G = k/4 lanes
// per sample, lane l holds dims [4l, 4l+4); VW = 1: G = power of two >= k
// lanes, lane j = dim j.  A lane keeps the rows of up to TMAXF fields in
// registers: with F <= TMAXF the rows are read once; beyond it (sum / mean
// only) the first pass accumulates S and sum e^2 and a second pass gathers
// the rows again, chunk by chunk, for the gradient blocks.  MAXP: the 'max'
// pool with the arg-max pair (i*, j*) tracked per dim — per first field c the
// best partner d > c (strict >, so the first d wins a tie), then the best c
// (strict > again): the first pair in row-major order.
template <int G, int VW, int KIND, bool MAXP>
__global__ __launch_bounds__(256) void afm_train_kernel(AfmTrainArgs a) {
  typedef Ids<KIND> I;
  constexpr int CH = TMAXF;
  const int64_t b = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
  const int l = threadIdx.x & (G - 1);
  const bool valid = b < a.batch;
  const int64_t bb = valid ? b : a.batch - 1;
  const bool lane_ok = VW * l < a.k;
  const int jj = lane_ok ? VW * l : 0;  // first dim of this lane
  float e[CH][VW];
  uint32_t okm = 0;  // bit u: field c0 + u of the chunk in e has a valid id
  bool bad = false;
  auto load_chunk = [&](int c0) {
    int64_t row[CH];
    okm = 0;
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      const int c = c0 + u < a.F ? c0 + u : a.F - 1;
      int64_t id;
      const bool ok = I::decode(I::load(a.ids, bb * a.id_stride + c), a.vocab[c], id) && c0 + u < a.F;
      bad |= c0 + u < a.F && !ok;
      okm |= ok ? 1u << u : 0u;
      row[u] = a.offs[c] + id;
    }
#pragma unroll
    for (int u = 0; u < CH; ++u) load_row<VW>(a.table + row[u] * a.k + jj, e[u]);
#pragma unroll
    for (int u = 0; u < CH; ++u)
      if (!(okm >> u & 1)) {
#pragma unroll
        for (int t = 0; t < VW; ++t) e[u][t] = 0.f;
      }
  };
  float s[VW], q[VW], pooled[VW];
#pragma unroll
  for (int t = 0; t < VW; ++t) s[t] = q[t] = pooled[t] = 0.f;
  for (int c0 = 0; c0 < a.F; c0 += CH) {
    load_chunk(c0);
    if constexpr (!MAXP) {
#pragma unroll
      for (int u = 0; u < CH; ++u)
#pragma unroll
        for (int t = 0; t < VW; ++t) {
          s[t] += e[u][t];
          q[t] += e[u][t] * e[u][t];
        }
    }
  }
  if (bad && valid && lane_ok) flag_error(a.err);
  const float pscale = a.mode == 1 && a.F >= 2 ? 1.0f / (0.5f * (float)a.F * (float)(a.F - 1)) : 1.0f;  // 1 / P
  int ai[VW], aj[VW];  // MAXP: the arg-max pair per dim
  if constexpr (MAXP) {
#pragma unroll
    for (int t = 0; t < VW; ++t) ai[t] = 0, aj[t] = 1;
#pragma unroll
    for (int c = 0; c + 1 < CH; ++c)
      if (c + 1 < a.F) {
        float bm[VW];
        int bd[VW];
#pragma unroll
        for (int t = 0; t < VW; ++t) bm[t] = e[c][t] * e[c + 1][t], bd[t] = c + 1;
#pragma unroll
        for (int d = c + 2; d < CH; ++d)
          if (d < a.F) {
#pragma unroll
            for (int t = 0; t < VW; ++t) {
              const float p = e[c][t] * e[d][t];
              const bool up = p > bm[t];
              bm[t] = up ? p : bm[t];
              bd[t] = up ? d : bd[t];
            }
          }
#pragma unroll
        for (int t = 0; t < VW; ++t) {
          const bool up = c == 0 || bm[t] > pooled[t];
          pooled[t] = up ? bm[t] : pooled[t];
          ai[t] = up ? c : ai[t];
          aj[t] = up ? bd[t] : aj[t];
        }
      }
  } else {
    if (a.F >= 2) {
      // the forward's arithmetic (s * s - q contracts to fma(s, s, -q)); one field has no pair: exactly 0
#pragma unroll
      for (int t = 0; t < VW; ++t) {
        pooled[t] = 0.5f * (s[t] * s[t] - q[t]);
        if (a.mode == 1) pooled[t] = pooled[t] * pscale;
      }
    }
  }
  float w[VW];
#pragma unroll
  for (int t = 0; t < VW; ++t) w[t] = 0.f;
  if (lane_ok) {
    if constexpr (VW == 4) {
      const floatx4 hw = *reinterpret_cast<const floatx4*>(a.head_w + jj);
      w[0] = hw[0], w[1] = hw[1], w[2] = hw[2], w[3] = hw[3];
    } else {
      w[0] = a.head_w[jj];
    }
  }
  float y;
  if constexpr (VW == 4) y = (pooled[0] * w[0] + pooled[1] * w[1]) + (pooled[2] * w[2] + pooled[3] * w[3]);
  else y = pooled[0] * w[0];
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) y += __shfl_xor(y, o, G);
  y += a.head_b[0];
  const float g = afm_head(a, y, bb, valid && l == 0);
  if (!valid || !lane_ok) return;  // no barrier below
  store_row<VW>(a.pooled + b * a.pooled_stride + jj, pooled, a.vec_out);
  float dx[VW];
#pragma unroll
  for (int t = 0; t < VW; ++t) dx[t] = (a.F >= 2 ? g * pscale : 0.f) * w[t];
  float* drow = a.drows + b * a.drows_stride + jj;
  if constexpr (MAXP) {
    // the partners' values e[i*], e[j*] per dim (select chains: the registers cannot be indexed by a lane value)
    float ga[VW], gb[VW];
#pragma unroll
    for (int t = 0; t < VW; ++t) {
      float va = 0.f, vb = 0.f;
#pragma unroll
      for (int f = 0; f < CH; ++f) {
        va = ai[t] == f ? e[f][t] : va;
        vb = aj[t] == f ? e[f][t] : vb;
      }
      ga[t] = dx[t] * vb;  // dL/de_{i*}
      gb[t] = dx[t] * va;  // dL/de_{j*}
    }
#pragma unroll
    for (int u = 0; u < CH; ++u)
      if (u < a.F) {
        const bool ok = okm >> u & 1;
        float o[VW];
#pragma unroll
        for (int t = 0; t < VW; ++t) o[t] = !ok ? 0.f : ai[t] == u ? ga[t] : aj[t] == u ? gb[t] : 0.f;
        store_row<VW>(drow + u * a.k, o, a.vec_out);
      }
  } else {
    for (int c0 = 0; c0 < a.F; c0 += CH) {
      if (a.F > CH) load_chunk(c0);  // second pass: the chunk's rows again
#pragma unroll
      for (int u = 0; u < CH; ++u)
        if (c0 + u < a.F) {
          const bool ok = okm >> u & 1;
          float o[VW];
#pragma unroll
          for (int t = 0; t < VW; ++t) o[t] = ok ? dx[t] * (s[t] - e[u][t]) : 0.f;
          store_row<VW>(drow + (int64_t)(c0 + u) * a.k, o, a.vec_out);
        }
    }
  }
}

// Sum / mean, float4 lanes: pair_pool_ksplit's field split (interact.hip).
// NWP waves per workgroup split the fields (wave w takes fields w, w+NWP,
// ...: its ids first, then all its rows in flight) and KEEP their rows; the
// partial S and sum e^2 go through LDS, every wave adds the NWP partials in
// wave order (so all hold the same S), computes the head redundantly (one
// G-lane reduction and two exps) and writes the gradient blocks of its own
// fields.  Wave 0 writes pooled / prob / g / loss.  F > 32: a second pass
// gathers each chunk's rows again.
template <int G, int KIND, int NWP>
__global__ __launch_bounds__(NWP * 64) void afm_train_ksplit(AfmTrainArgs a) {
  typedef Ids<KIND> I;
  constexpr int CH = (TMAXF + NWP - 1) / NWP;  // fields per wave and pass
  __shared__ floatx4 sp[NWP][64], qp[NWP][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t b = (int64_t)blockIdx.x * (64 / G) + lane / G;
  const int l = lane & (G - 1);
  const bool valid = b < a.batch;
  const int64_t bb = valid ? b : a.batch - 1;
  const bool lane_ok = 4 * l < a.k;
  const int jj = lane_ok ? 4 * l : 0;
  const floatx4 zero = {0.f, 0.f, 0.f, 0.f};
  floatx4 v[CH];
  bool okc[CH];
  bool bad = false;
  auto load_chunk = [&](int c0) {
    int64_t row[CH];
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      const int cu = c0 + NWP * u;
      const int c = cu < a.F ? cu : a.F - 1;
      int64_t id;
      okc[u] = I::decode(I::load(a.ids, bb * a.id_stride + c), a.vocab[c], id) && cu < a.F;
      bad |= cu < a.F && !okc[u];
      row[u] = a.offs[c] + id;
    }
#pragma unroll
    for (int u = 0; u < CH; ++u)
      v[u] = __builtin_nontemporal_load(reinterpret_cast<const floatx4*>(a.table + row[u] * a.k + jj));
#pragma unroll
    for (int u = 0; u < CH; ++u) v[u] = okc[u] ? v[u] : zero;
  };
  floatx4 s = zero, q = zero;
  for (int c0 = w; c0 < a.F; c0 += NWP * CH) {
    load_chunk(c0);
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      s += v[u];
      q += v[u] * v[u];
    }
  }
  if (bad && valid && lane_ok) flag_error(a.err);
  sp[w][lane] = s;
  qp[w][lane] = q;
  __syncthreads();
  s = sp[0][lane];
  q = qp[0][lane];
#pragma unroll
  for (int ww = 1; ww < NWP; ++ww) {
    s += sp[ww][lane];
    q += qp[ww][lane];
  }
  const float pscale = a.mode == 1 && a.F >= 2 ? 1.0f / (0.5f * (float)a.F * (float)(a.F - 1)) : 1.0f;  // 1 / P
  floatx4 pooled = a.F >= 2 ? 0.5f * (s * s - q) : zero;  // one field: no pair, exactly 0
  if (a.mode == 1) pooled = pooled * pscale;
  const floatx4 hw = lane_ok ? *reinterpret_cast<const floatx4*>(a.head_w + jj) : zero;
  const floatx4 ph = pooled * hw;
  float y = (ph[0] + ph[1]) + (ph[2] + ph[3]);
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) y += __shfl_xor(y, o, G);
  y += a.head_b[0];
  const float g = afm_head(a, y, bb, valid && l == 0 && w == 0);
  if (!valid || !lane_ok) return;  // no barrier below
  if (w == 0) {
    const float po[4] = {pooled[0], pooled[1], pooled[2], pooled[3]};
    store_row<4>(a.pooled + b * a.pooled_stride + jj, po, a.vec_out);
  }
  const floatx4 dx = (a.F >= 2 ? g * pscale : 0.f) * hw;
  float* drow = a.drows + b * a.drows_stride + jj;
  for (int c0 = w; c0 < a.F; c0 += NWP * CH) {
    if (a.F > NWP * CH) load_chunk(c0);  // second pass: the chunk's rows again
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      const int cu = c0 + NWP * u;
      if (cu < a.F) {
        const floatx4 d = okc[u] ? dx * (s - v[u]) : zero;
        const float o[4] = {d[0], d[1], d[2], d[3]};
        store_row<4>(drow + (int64_t)cu * a.k, o, a.vec_out);
      }
    }
  }
}

}  // namespace rs

using namespace rs;

extern "C" int rs_afm_train_fwd(const void* ids, int id_kind, int64_t id_stride, const float* table,
                                const int64_t* field_offsets, const int64_t* field_vocab, int n_fields, int k,
                                int mode, const float* head_w, const float* head_b, int n_sigmoid,
                                const float* labels, int64_t batch, float* pooled, int64_t pooled_stride,
                                float* prob, float* g, float* loss, float* drows, int64_t drows_stride,
                                int* err_flag, rs_stream_t stream) {
  if (batch == 0) return RS_OK;  // empty batch: nothing to launch
  RS_REQUIRE(batch > 0 && n_fields >= 1 && k >= 1 && k <= 64 && mode >= 0 && mode <= 2,
             "rs_afm_train_fwd: bad shape (1 <= k <= 64, mode 0..2)");
  RS_REQUIRE(n_sigmoid == 1 || n_sigmoid == 2, "rs_afm_train_fwd: n_sigmoid must be 1 or 2");
  RS_REQUIRE(mode != 2 || n_fields <= TMAXF, "rs_afm_train_fwd: 'max' pooling supports at most %d fields", TMAXF);
  RS_REQUIRE(ids && table && field_offsets && field_vocab && head_w && head_b && labels,
             "rs_afm_train_fwd: null input pointer");
  RS_REQUIRE(pooled && g && drows, "rs_afm_train_fwd: null output pointer (pooled, g and drows are required)");
  RS_REQUIRE(pooled_stride >= k && drows_stride >= (int64_t)n_fields * k, "rs_afm_train_fwd: bad output layout");
  RS_REQUIRE(id_kind >= RS_ID_I32 && id_kind <= RS_ID_F32, "rs_afm_train_fwd: bad id_kind");
  const bool v4 = k % 4 == 0 && (uintptr_t)table % 16 == 0 && (uintptr_t)head_w % 16 == 0;
  const bool vec_out = (uintptr_t)pooled % 16 == 0 && (uintptr_t)drows % 16 == 0 && pooled_stride % 4 == 0 &&
                       drows_stride % 4 == 0;
  AfmTrainArgs a{ids, id_stride, table, field_offsets, field_vocab, n_fields, k, mode, head_w, head_b, n_sigmoid,
                 labels, batch, pooled, pooled_stride, prob, g, loss, drows, drows_stride, vec_out, err_flag};
  int G = 1;
  while (G * (v4 ? 4 : 1) < k) G <<= 1;
  const int nth = v4 ? 64 : 256;  // the forward's geometry (rs_embed_pair_pool_fwd)
  const unsigned grid = (unsigned)((batch * G + nth - 1) / nth);
  hipStream_t st = as_stream(stream);
  with_id_kind(id_kind, [&](auto K) {
    constexpr int KD = decltype(K)::value;
    auto go = [&](auto MX) {
      constexpr bool MAXP = decltype(MX)::value;
      if (v4) {
        if constexpr (MAXP) {  // float4 sum / mean runs the field-split kernel below
          switch (G) {
            case 1: afm_train_kernel<1, 4, KD, true><<<grid, nth, 0, st>>>(a); break;
            case 2: afm_train_kernel<2, 4, KD, true><<<grid, nth, 0, st>>>(a); break;
            case 4: afm_train_kernel<4, 4, KD, true><<<grid, nth, 0, st>>>(a); break;
            case 8: afm_train_kernel<8, 4, KD, true><<<grid, nth, 0, st>>>(a); break;
            default: afm_train_kernel<16, 4, KD, true><<<grid, nth, 0, st>>>(a); break;
          }
        }
      } else {
        switch (G) {
          case 1: afm_train_kernel<1, 1, KD, MAXP><<<grid, nth, 0, st>>>(a); break;
          case 2: afm_train_kernel<2, 1, KD, MAXP><<<grid, nth, 0, st>>>(a); break;
          case 4: afm_train_kernel<4, 1, KD, MAXP><<<grid, nth, 0, st>>>(a); break;
          case 8: afm_train_kernel<8, 1, KD, MAXP><<<grid, nth, 0, st>>>(a); break;
          case 16: afm_train_kernel<16, 1, KD, MAXP><<<grid, nth, 0, st>>>(a); break;
          case 32: afm_train_kernel<32, 1, KD, MAXP><<<grid, nth, 0, st>>>(a); break;
          default: afm_train_kernel<64, 1, KD, MAXP><<<grid, nth, 0, st>>>(a); break;
        }
      }
    };
    if (mode != 2 && v4) {
      const unsigned g2 = (unsigned)((batch + 64 / G - 1) / (64 / G));
      constexpr int NWP = 8;  // the forward's split: <= 4 fields per wave at F = 26
      switch (G) {
        case 1: afm_train_ksplit<1, KD, NWP><<<g2, NWP * 64, 0, st>>>(a); break;
        case 2: afm_train_ksplit<2, KD, NWP><<<g2, NWP * 64, 0, st>>>(a); break;
        case 4: afm_train_ksplit<4, KD, NWP><<<g2, NWP * 64, 0, st>>>(a); break;
        case 8: afm_train_ksplit<8, KD, NWP><<<g2, NWP * 64, 0, st>>>(a); break;
        default: afm_train_ksplit<16, KD, NWP><<<g2, NWP * 64, 0, st>>>(a); break;
      }
    } else if (mode != 2) {
      go(std::false_type());
    } else {
      go(std::true_type());
    }
  });
  return launch_status("rs_afm_train_fwd");
}
