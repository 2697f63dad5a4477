// embed_gather.hip — the plain embedding lookup (rs_embed_gather: x = [dense |
// emb]) and the FM model on one-hot input (rs_fm_onehot_fwd).
//
// Reference semantics:
//   EmbedLayer.call            algorithm/deep_learning/layer/core.py:273-280
//   DeepFM x = [dense | emb]   algorithm/deep_learning/model/deepFM.py:24-26
//   FM model (one-hot input)   algorithm/deep_learning/model/fm.py:19-23,
//                              utils/dataset.py:47-48 (get_dummies layout)
#include "embed_fm.hpp"
#include "rs_common.hpp"

namespace rs {

// -------------------------------------------------------------- gather
struct GatherArgs {
  const void* ids;
  int64_t id_stride;
  const float* dense;
  int64_t dense_stride;
  int nd;
  const float* table;
  const int64_t* offs;
  const int64_t* vocab;
  int F, k;
  float* out;
  int64_t out_stride;
  int64_t batch;
  int* err;
  int vec_store;
};

// Thread t handles chunk q of field c of sample b (VW floats); consecutive
// threads walk a row then the next field, so 4 threads read one 64-B row.
template <int VW, int KIND>
__global__ __launch_bounds__(256) void embed_gather_kernel(GatherArgs a) {
  typedef Ids<KIND> I;
  const uint32_t KQ = a.k / VW;
  const uint32_t per_row = (uint32_t)a.F * KQ;
  const uint32_t total = (uint32_t)a.batch * per_row;
  bool bad = false;
  for (uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
    const uint32_t bb = idx / per_row, r = idx - bb * per_row;
    const uint32_t c = r / KQ, q = r - c * KQ;
    const int64_t b = bb;
    int64_t id;
    const bool ok = I::decode(I::load(a.ids, b * a.id_stride + c), a.vocab[c], id);
    bad |= !ok;
    Chunk<VW> x;
    x.load(a.table + (a.offs[c] + id) * a.k + q * VW);
    float* dst = a.out + b * a.out_stride + a.nd + c * a.k + q * VW;
    if constexpr (VW == 4) {
      if (a.vec_store) {
        *reinterpret_cast<floatx4*>(dst) =
            ok ? floatx4{x.v[0], x.v[1], x.v[2], x.v[3]} : floatx4{0.f, 0.f, 0.f, 0.f};
        continue;
      }
    }
#pragma unroll
    for (int t = 0; t < VW; ++t) dst[t] = ok ? x.v[t] : 0.f;
  }
  if (bad) flag_error(a.err);
  if (a.nd > 0) {
    const uint32_t tot = (uint32_t)a.batch * a.nd;
    for (uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x; idx < tot; idx += gridDim.x * blockDim.x) {
      const uint32_t bb = idx / a.nd, e = idx - bb * a.nd;
      a.out[(int64_t)bb * a.out_stride + e] = a.dense[(int64_t)bb * a.dense_stride + e];
    }
  }
}

// ------------------------------------------------------ FM one-hot gather
struct OnehotArgs {
  const void* ids;
  int64_t id_stride;
  const float* dense;
  int64_t dense_stride;
  int nd;
  const int64_t* offs;
  const int64_t* vocab;
  int F;
  const float* w1;
  const float* w0;
  const float* v;
  int kfm;
  float* logit;
  int64_t batch;
  int* err;
};

// G lanes per sample (lane f owns latent factor f); 256/G samples per block.
template <int G, int KIND>
__global__ __launch_bounds__(256) void fm_onehot_kernel(OnehotArgs a) {
  typedef Ids<KIND> I;
  const int f = threadIdx.x % G;
  const int64_t bt = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
  const bool valid = bt < a.batch;
  const int64_t b = valid ? bt : a.batch - 1;
  const int fc = f < a.kfm ? f : 0;
  float s = 0.f, q = 0.f, lin = 0.f;
  bool bad = false;
  for (int i = 0; i < a.nd; ++i) {
    const float x = a.dense[b * a.dense_stride + i];
    const float vf = f < a.kfm ? a.v[(int64_t)i * a.kfm + fc] : 0.f;
    s = fmaf(x, vf, s);
    q = fmaf(x * x, vf * vf, q);
    lin = fmaf(x, a.w1[i], lin);
  }
  for (int c = 0; c < a.F; ++c) {
    int64_t id;
    const bool ok = I::decode(I::load(a.ids, b * a.id_stride + c), a.vocab[c], id);
    bad |= !ok;
    const int64_t row = a.nd + a.offs[c] + id;
    const float vr = a.v[row * a.kfm + fc];
    const float wr = a.w1[row];
    const float vf = (ok && f < a.kfm) ? vr : 0.f;
    s += vf;
    q = fmaf(vf, vf, q);
    lin += ok ? wr : 0.f;
  }
  float term = (f < a.kfm) ? (s * s - q) : 0.f;
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) term += __shfl_xor(term, o, G);
  if (bad && valid && f == 0) flag_error(a.err);
  if (valid && f == 0) a.logit[b] = (lin + a.w0[0]) + 0.5f * term;
}

}  // namespace rs

using namespace rs;

extern "C" int rs_embed_gather(const void* ids, int id_kind, int64_t id_stride, const float* dense,
                               int64_t dense_stride, int nd, const float* table, const int64_t* field_offsets,
                               const int64_t* field_vocab, int n_fields, int k, float* out, int64_t out_stride,
                               int64_t batch, int* err_flag, rs_stream_t stream) {
  if (batch == 0) return RS_OK;  // empty batch: nothing to launch (null data pointers allowed)
  RS_REQUIRE(batch >= 0 && nd >= 0 && n_fields >= 0, "rs_embed_gather: bad shape");
  RS_REQUIRE(out && (nd == 0 || dense), "rs_embed_gather: null pointer");
  RS_REQUIRE(n_fields == 0 || (ids && table && field_offsets && field_vocab && k >= 1),
             "rs_embed_gather: sparse inputs missing");
  RS_REQUIRE(id_kind >= RS_ID_I32 && id_kind <= RS_ID_F32, "rs_embed_gather: bad id_kind");
  RS_REQUIRE(out_stride >= nd + (int64_t)n_fields * k, "rs_embed_gather: out_stride too small");
  RS_REQUIRE(batch * (int64_t)(n_fields * (int64_t)k + nd) < (int64_t)1 << 31,
             "rs_embed_gather: batch*row too large for one launch");
  GatherArgs a{ids, id_stride, dense, dense_stride, nd, table, field_offsets, field_vocab,
               n_fields, k, out, out_stride, batch, err_flag, 0};
  hipStream_t st = as_stream(stream);
  const bool vec_src = (k % 4 == 0) && ((uintptr_t)table % 16 == 0);
  if (n_fields == 0) {
    a.F = 0;
    a.k = 4;
    embed_gather_kernel<4, 0><<<grid_for(batch * nd, 256, 8192), 256, 0, st>>>(a);
  } else if (vec_src) {
    a.vec_store = ((uintptr_t)out % 16 == 0) && (out_stride % 4 == 0) && (nd % 4 == 0);
    const int64_t work = batch * n_fields * (k / 4);
    with_id_kind(id_kind, [&](auto K) {
      embed_gather_kernel<4, decltype(K)::value>
          <<<grid_for(work > batch * nd ? work : batch * nd, 256, 8192), 256, 0, st>>>(a);
    });
  } else {
    const int64_t work = batch * n_fields * k;
    with_id_kind(id_kind, [&](auto K) {
      embed_gather_kernel<1, decltype(K)::value>
          <<<grid_for(work > batch * nd ? work : batch * nd, 256, 8192), 256, 0, st>>>(a);
    });
  }
  return launch_status("rs_embed_gather");
}

extern "C" int rs_fm_onehot_fwd(const void* ids, int id_kind, int64_t id_stride, const float* dense,
                                int64_t dense_stride, int nd, const int64_t* field_offsets,
                                const int64_t* field_vocab, int n_fields, const float* w1, const float* w0,
                                const float* v, int kfm, float* logit, int64_t batch, int* err_flag,
                                rs_stream_t stream) {
  if (batch == 0) return RS_OK;  // empty batch: nothing to launch (null data pointers allowed)
  RS_REQUIRE(batch >= 0 && nd >= 0 && n_fields >= 0 && kfm >= 1 && kfm <= 64, "rs_fm_onehot_fwd: bad shape");
  RS_REQUIRE(w1 && w0 && v && logit && (nd == 0 || dense), "rs_fm_onehot_fwd: null pointer");
  RS_REQUIRE(n_fields == 0 || (ids && field_offsets && field_vocab), "rs_fm_onehot_fwd: sparse inputs missing");
  RS_REQUIRE(id_kind >= RS_ID_I32 && id_kind <= RS_ID_F32, "rs_fm_onehot_fwd: bad id_kind");
  OnehotArgs a{ids, id_stride, dense, dense_stride, nd, field_offsets, field_vocab, n_fields,
               w1, w0, v, kfm, logit, batch, err_flag};
  hipStream_t st = as_stream(stream);
  int G = 4;
  while (G < kfm) G *= 2;
  const int spb = 256 / G;
  const unsigned grid = (unsigned)((batch + spb - 1) / spb);
  with_id_kind(id_kind, [&](auto K) {
    constexpr int KI = decltype(K)::value;
    switch (G) {
      case 4: fm_onehot_kernel<4, KI><<<grid, 256, 0, st>>>(a); break;
      case 8: fm_onehot_kernel<8, KI><<<grid, 256, 0, st>>>(a); break;
      case 16: fm_onehot_kernel<16, KI><<<grid, 256, 0, st>>>(a); break;
      case 32: fm_onehot_kernel<32, KI><<<grid, 256, 0, st>>>(a); break;
      default: fm_onehot_kernel<64, KI><<<grid, 256, 0, st>>>(a); break;
    }
  });
  return launch_status("rs_fm_onehot_fwd");
}
