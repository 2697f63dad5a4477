// wide.hip — WideLayer (layer/interaction.py:11-26: w0 + x @ w) on the compact
// form of Wide&Deep's wide input (model/wideDeep.py:22-34 with
// utils/dataset.py:64-66): x = [dense (nd) | dense again (nd) | one-hot], the
// one-hot block holding exactly one 1 per field at column 2 nd + offset_c +
// id(b, c).  A gather of one scalar per field, not a matmul over the one-hot
// width; no one-hot matrix is formed.
#include "rs_common.hpp"

namespace rs {

struct WideArgs {
  const void* ids;
  int64_t id_stride;
  const float* dense;
  int64_t dense_stride;
  int nd;
  const int64_t* offs;
  const int64_t* width;
  int F;
  const float* w;
  const float* w0;
  float* logit;
  int64_t batch;
  int* err;
};

// one sample per thread; the sum runs in column order of the compact form
// (w0, the dense columns, then the fields)
template <int KIND>
__global__ __launch_bounds__(256) void wide_onehot_kernel(WideArgs a) {
  typedef Ids<KIND> I;
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= a.batch) return;
  float s = a.w0[0];
  for (int j = 0; j < a.nd; ++j) s = fmaf(a.dense[b * a.dense_stride + j], a.w[j] + a.w[a.nd + j], s);
  bool bad = false;
  for (int c = 0; c < a.F; ++c) {
    int64_t id;
    const bool ok = I::decode(I::load(a.ids, b * a.id_stride + c), a.width[c], id);
    s += ok ? a.w[2 * (int64_t)a.nd + a.offs[c] + id] : 0.f;
    bad |= !ok;
  }
  if (bad) flag_error(a.err);
  a.logit[b] = s;
}

}  // namespace rs

using namespace rs;

extern "C" int rs_wide_onehot_fwd(const void* ids, int id_kind, int64_t id_stride, const float* dense,
                                  int64_t dense_stride, int nd, const int64_t* field_offsets,
                                  const int64_t* field_widths, int n_fields, const float* w, const float* w0,
                                  float* logit, int64_t batch, int* err_flag, rs_stream_t stream) {
  if (batch == 0) return RS_OK;  // empty batch: nothing to launch (null data pointers allowed)
  RS_REQUIRE(batch >= 0 && nd >= 0 && n_fields >= 0, "rs_wide_onehot_fwd: bad shape");
  RS_REQUIRE(w && w0 && logit && (nd == 0 || dense), "rs_wide_onehot_fwd: null pointer");
  RS_REQUIRE(n_fields == 0 || (ids && field_offsets && field_widths), "rs_wide_onehot_fwd: sparse inputs missing");
  RS_REQUIRE(id_kind >= RS_ID_I32 && id_kind <= RS_ID_F32, "rs_wide_onehot_fwd: bad id_kind");
  RS_REQUIRE((n_fields == 0 || id_stride >= n_fields) && (nd == 0 || dense_stride >= nd),
             "rs_wide_onehot_fwd: id_stride / dense_stride smaller than the width");
  const int64_t grid = (batch + 255) / 256;
  RS_REQUIRE(grid < (1ll << 31), "rs_wide_onehot_fwd: batch too large");
  WideArgs a{ids, id_stride, dense, dense_stride, nd, field_offsets, field_widths, n_fields, w, w0, logit, batch,
             err_flag};
  with_id_kind(id_kind, [&](auto K) {
    wide_onehot_kernel<decltype(K)::value><<<(unsigned)grid, 256, 0, as_stream(stream)>>>(a);
  });
  return launch_status("rs_wide_onehot_fwd");
}
