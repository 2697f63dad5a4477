// fnn_train.hip — stage 2 of FNN (model/fnn.py:53-63): the first Dense layer
// of the tower on x (.) v, forward and SGD, on the compact batch.
//
// v is a constant of the second fit; W1 [n*k, H1] (viewed [n, k, H1]) moves
// every step, so there is no projected table here.  The B*A lookups (A = nd +
// F: dense feature j is row j with value dense[b, j], field c is row nd +
// off_c + id with value 1) are sorted once by row (radix_sort.hpp, stable),
// and the one sort serves both directions:
//   rs_fnn_train_fwd  per distinct row u of the batch Pu[u] = v[f_u] @ W1[f_u]
//                     (each touched slab read once, however many samples
//                     share it), then z1[b] = b1 + sum_a x_a Pu[slot(b, a)];
//   rs_fnn_w1_sgd     dz1 = d_a1 * mult * [mask > 0]; per distinct row
//                     g_f = sum over its lookups, in lookup order, of
//                     x * dz1[b] (seg_piece / seg_cross, rs_common.hpp: chunk
//                     pieces added in chunk order, no atomics), then
//                     W1[f][j, :] -= lr * v[f, j] * g_f in place.
// dW1 is rank 1 per row and zero on every row no sample touched; those slabs
// are never written.  No [B, n*k], [n*k, H1] or per-lookup [k, H1] buffer.
#include "radix_sort.hpp"
#include "rs_common.hpp"

namespace rs {

// workspace layout (bytes, 256-B aligned pieces); n = batch * (nd + n_fields)
struct FnnWs {
  int64_t key_in, key_out, val_in, val_out, scan, lslot, ustart, part, sort, pu, total;
};

static int64_t fnn_al(int64_t x) { return (x + 255) / 256 * 256; }

static FnnWs fnn_ws(int64_t batch, int nd, int n_fields, int64_t n_rows, int H1) {
  FnnWs w{};
  const int64_t n = batch * (nd + n_fields);
  const int64_t umax = std::min<int64_t>(n, n_rows);  // distinct rows of a batch
  int64_t o = 0;
  w.key_in = o; o = fnn_al(o + n * 4);
  w.key_out = o; o = fnn_al(o + n * 4);
  w.val_in = o; o = fnn_al(o + n * 4);
  w.val_out = o; o = fnn_al(o + n * 4);
  w.scan = o; o = fnn_al(o + n * 4);    // heads so far, inclusive: slot of position p = scan[p] - 1
  w.lslot = o; o = fnn_al(o + n * 4);   // slot of lookup j (-1: a bad id)
  w.ustart = o; o = fnn_al(o + n * 4);  // first sorted position of slot u
  w.part = o; o = fnn_al(o + (n + 2 * (int64_t)H1) * 4);  // >= 2 * nchunk * H1 floats (seg_chunk(H1) >= 4 H1)
  w.sort = o; o = fnn_al(o + std::max(sort_pairs_ws_bytes(n), scan_ws_bytes(n)));
  w.pu = o; o = fnn_al(o + std::max<int64_t>(umax, 1) * H1 * 4);
  w.total = o;
  return w;
}

struct FnnTrainArgs {
  const void* ids;
  int64_t id_stride;
  const float* dense;
  int64_t ds;
  int nd;
  const int64_t* offs;
  const int64_t* vocab;
  int F;
  const float* v;  // [n_rows, k]
  float* W1;       // [n_rows, k, H1]
  int64_t n_rows;
  int k, H1;
  int64_t B, n;  // n = B * (nd + F) lookups
  uint32_t* key_in;
  uint32_t* key_out;
  uint32_t* val_in;
  uint32_t* val_out;
  int32_t* scan;
  int32_t* lslot;
  int32_t* ustart;
  float* part;
  float* pu;
  int* err;
};

// lookup j = b * A + a: key = its row (0xffffffff: a bad id, sorts last)
template <int KIND>
__global__ __launch_bounds__(256) void fnn_keys_kernel(FnnTrainArgs a) {
  typedef Ids<KIND> I;
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.n) return;
  const int A = a.nd + a.F;
  const int64_t b = j / A;
  const int c = (int)(j - b * A);
  uint32_t key = (uint32_t)c;
  if (c >= a.nd) {
    int64_t id;
    bool ok = I::decode(I::load(a.ids, b * a.id_stride + (c - a.nd)), a.vocab[c - a.nd], id);
    const int64_t row = a.nd + a.offs[c - a.nd] + id;
    ok = ok && row < a.n_rows;
    if (!ok) flag_error(a.err);
    key = ok ? (uint32_t)row : 0xffffffffu;
  }
  a.key_in[j] = key;
  a.val_in[j] = (uint32_t)j;
}

__global__ __launch_bounds__(256) void fnn_heads_kernel(FnnTrainArgs a) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.n) return;
  const uint32_t r = a.key_out[p];
  a.scan[p] = (r != 0xffffffffu && (p == 0 || a.key_out[p - 1] != r)) ? 1 : 0;
}

__global__ __launch_bounds__(256) void fnn_slots_kernel(FnnTrainArgs a) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.n) return;
  const uint32_t r = a.key_out[p];
  const bool valid = r != 0xffffffffu;
  const int32_t slot = a.scan[p] - 1;
  a.lslot[a.val_out[p]] = valid ? slot : -1;
  if (valid && (p == 0 || a.key_out[p - 1] != r)) a.ustart[slot] = (int32_t)p;
}

template <int V>
__device__ __forceinline__ void fnn_st(float* dst, const float (&v)[V]) {
  if constexpr (V == 4) {
    floatx4 t = {v[0], v[1], v[2], v[3]};
    *reinterpret_cast<floatx4*>(dst) = t;
  } else {
    dst[0] = v[0];
  }
}

// Pu[u, :] = v[f_u, :] @ W1[f_u] (j in order, fmaf chain, as rs_fnn_project):
// waves stride over the distinct rows; the count comes from device memory.
template <int V>
__global__ __launch_bounds__(256) void fnn_pu_kernel(FnnTrainArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t U = a.scan[a.n - 1];
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < U; u += nw) {
    const int64_t f = a.key_out[a.ustart[u]];
    const float* vr = a.v + f * a.k;
    for (int c = V * lane; c < a.H1; c += 64 * V) {
      const float* wr = a.W1 + f * a.k * (int64_t)a.H1 + c;
      float acc[V];
#pragma unroll
      for (int q = 0; q < V; ++q) acc[q] = 0.f;
      for (int j0 = 0; j0 < a.k; j0 += 4) {
        Chunk<V> w[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) w[t].load(wr + (int64_t)(j0 + t < a.k ? j0 + t : a.k - 1) * a.H1);
#pragma unroll
        for (int t = 0; t < 4; ++t)
          if (j0 + t < a.k) {
            const float vj = vr[j0 + t];
#pragma unroll
            for (int q = 0; q < V; ++q) acc[q] = fmaf(vj, w[t].v[q], acc[q]);
          }
      }
      fnn_st<V>(a.pu + u * a.H1 + c, acc);
    }
  }
}

// z1[b] = b1 + sum_a x_a Pu[slot(b, a)], a in order; act applied when asked.
template <int V>
__global__ __launch_bounds__(256) void fnn_z1_kernel(FnnTrainArgs a, const float* __restrict__ b1, int act,
                                                     float* __restrict__ out, int64_t os) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B) return;  // wave-uniform
  const int A = a.nd + a.F;
  for (int c = V * lane; c < a.H1; c += 64 * V) {
    float acc[V];
    Chunk<V> t;
    t.load(b1 + c);
#pragma unroll
    for (int q = 0; q < V; ++q) acc[q] = t.v[q];
    for (int a0 = 0; a0 < A; a0 += 4) {
      Chunk<V> p[4];
      float x[4];
      bool ok[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = a0 + u < A ? a0 + u : A - 1;
        const int32_t s = a.lslot[b * A + i];
        ok[u] = a0 + u < A && s >= 0;
        x[u] = i < a.nd ? a.dense[b * a.ds + i] : 1.f;
        p[u].load(a.pu + (int64_t)(s >= 0 ? s : 0) * a.H1 + c);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (ok[u]) {
          if (a0 + u < a.nd) {
#pragma unroll
            for (int q = 0; q < V; ++q) acc[q] = fmaf(x[u], p[u].v[q], acc[q]);
          } else {
#pragma unroll
            for (int q = 0; q < V; ++q) acc[q] += p[u].v[q];
          }
        }
    }
#pragma unroll
    for (int q = 0; q < V; ++q) {
      if (act == RS_ACT_RELU) acc[q] = fmaxf(acc[q], 0.f);
      else if (act == RS_ACT_SIGMOID) acc[q] = sigmoidf_(acc[q]);
    }
    fnn_st<V>(out + b * os + c, acc);
  }
}

// dz1 = d_a1 (* mult) where mask > 0 (no mask: everywhere)
__global__ __launch_bounds__(256) void fnn_dz1_kernel(const float* __restrict__ d, int64_t ldd,
                                                      const float* __restrict__ mult, int64_t ldm,
                                                      const float* __restrict__ mask, int64_t ldk, int64_t B, int H1,
                                                      float* __restrict__ dz1) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= B * H1) return;
  const int64_t b = t / H1;
  const int c = (int)(t - b * H1);
  float x = d[b * ldd + c];
  if (mult) x *= mult[b * ldm + c];
  if (mask && !(mask[b * ldk + c] > 0.f)) x = 0.f;
  dz1[t] = x;
}

struct FnnSgdArgs {
  FnnTrainArgs t;
  const float* dz1;  // [B, H1]
  float lr;
  float* g_out;  // [U, H1] by slot, or null
  int64_t C;
};

__device__ __forceinline__ void fnn_apply_row(const FnnSgdArgs& s, int64_t p, uint32_t r, int c, float g) {
  const FnnTrainArgs& a = s.t;
  if (s.g_out) s.g_out[(int64_t)(a.scan[p] - 1) * a.H1 + c] = g;
  if (a.W1) {
    float* w = a.W1 + (int64_t)r * a.k * a.H1 + c;
    const float* vr = a.v + (int64_t)r * a.k;
    for (int j = 0; j < a.k; ++j) w[(int64_t)j * a.H1] -= s.lr * (vr[j] * g);
  }
}

// one thread per (sorted position, column)
__global__ __launch_bounds__(256) void fnn_piece_kernel(FnnSgdArgs s) {
  const FnnTrainArgs& a = s.t;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= a.n * a.H1) return;
  const int64_t p = t / a.H1;
  const int c = (int)(t - p * a.H1);
  const int A = a.nd + a.F;
  const int64_t nch = (a.n + s.C - 1) / s.C;
  uint32_t r;
  float acc;
  if (seg_piece<16>(a.key_out, a.n, s.C, p, a.H1, c,
                    [&](int64_t q) {
                      const int64_t j = a.val_out[q];
                      const int64_t b = j / A;
                      const int i = (int)(j - b * A);
                      const float d = s.dz1[b * a.H1 + c];
                      return i < a.nd ? a.dense[b * a.ds + i] * d : d;
                    },
                    a.part, a.part + nch * a.H1, r, acc))
    fnn_apply_row(s, p, r, c, acc);
}

__global__ __launch_bounds__(256) void fnn_cross_kernel(FnnSgdArgs s) {
  const FnnTrainArgs& a = s.t;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= a.n * a.H1) return;
  const int64_t p = t / a.H1;
  const int c = (int)(t - p * a.H1);
  const int64_t nch = (a.n + s.C - 1) / s.C;
  uint32_t r;
  float acc;
  if (seg_cross(a.key_out, a.n, s.C, p, a.H1, c, a.part, a.part + nch * a.H1, r, acc))
    fnn_apply_row(s, p, r, c, acc);
}

static bool fnn_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static int fnn_train_fill(const char* what, const void* ids, int id_kind, int64_t id_stride, const float* dense,
                          int64_t dense_stride, int nd, const int64_t* field_offsets, const int64_t* field_vocab,
                          int n_fields, const float* v, float* W1, int64_t n_rows, int k, int H1, int64_t batch,
                          void* workspace, int* err_flag, FnnTrainArgs& a) {
  RS_REQUIRE(batch > 0 && nd >= 0 && n_fields >= 0 && nd + n_fields >= 1 && k >= 1 && H1 >= 1 && n_rows >= nd,
             "%s: bad shape", what);
  const int64_t n = batch * (nd + n_fields);
  RS_REQUIRE(n_rows < 0xffffffffll && n < (1ll << 31) && n * H1 < (1ll << 38),
             "%s: rows must fit uint32, lookups int32", what);
  RS_REQUIRE(v && workspace && (nd == 0 || (dense && dense_stride >= nd)) &&
                 (n_fields == 0 || (ids && field_offsets && field_vocab && id_stride >= n_fields)),
             "%s: null pointer or short stride", what);
  RS_REQUIRE(id_kind >= RS_ID_I32 && id_kind <= RS_ID_F32, "%s: bad id_kind", what);
  const FnnWs w = fnn_ws(batch, nd, n_fields, n_rows, H1);
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  a = FnnTrainArgs{ids, id_stride, dense, dense_stride, nd, field_offsets, field_vocab, n_fields, v, W1, n_rows, k,
                   H1, batch, n,
                   reinterpret_cast<uint32_t*>(ws + w.key_in), reinterpret_cast<uint32_t*>(ws + w.key_out),
                   reinterpret_cast<uint32_t*>(ws + w.val_in), reinterpret_cast<uint32_t*>(ws + w.val_out),
                   reinterpret_cast<int32_t*>(ws + w.scan), reinterpret_cast<int32_t*>(ws + w.lslot),
                   reinterpret_cast<int32_t*>(ws + w.ustart), reinterpret_cast<float*>(ws + w.part),
                   reinterpret_cast<float*>(ws + w.pu), err_flag};
  return RS_OK;
}

}  // namespace rs

using namespace rs;

extern "C" int64_t rs_fnn_train_workspace_size(int64_t batch, int nd, int n_fields, int64_t n_rows, int H1) {
  if (batch < 0 || nd < 0 || n_fields < 0 || n_rows < 0 || H1 < 1) {
    set_error("rs_fnn_train_workspace_size: bad shape");
    return -1;
  }
  return fnn_ws(batch, nd, n_fields, n_rows, H1).total;
}

extern "C" int rs_fnn_train_fwd(const void* ids, int id_kind, int64_t id_stride, const float* dense,
                                int64_t dense_stride, int nd, const int64_t* field_offsets,
                                const int64_t* field_vocab, int n_fields, const float* v, const float* W1,
                                int64_t n_rows, int k, int H1, const float* b1, int act, float* out,
                                int64_t out_stride, int64_t batch, void* workspace, int* err_flag,
                                rs_stream_t stream) {
  if (batch == 0) return RS_OK;
  const char* what = "rs_fnn_train_fwd";
  FnnTrainArgs a;
  const int s = fnn_train_fill(what, ids, id_kind, id_stride, dense, dense_stride, nd, field_offsets, field_vocab,
                               n_fields, v, const_cast<float*>(W1), n_rows, k, H1, batch, workspace, err_flag, a);
  if (s != RS_OK) return s;
  RS_REQUIRE(W1 && b1 && out && out_stride >= H1, "%s: null pointer or short output", what);
  RS_REQUIRE(act == RS_ACT_NONE || act == RS_ACT_RELU || act == RS_ACT_SIGMOID,
             "%s: activation must be none, relu or sigmoid", what);
  hipStream_t st = as_stream(stream);
  const FnnWs w = fnn_ws(batch, nd, n_fields, n_rows, H1);
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  const unsigned gn = (unsigned)((a.n + 255) / 256);
  with_id_kind(id_kind, [&](auto K) { fnn_keys_kernel<decltype(K)::value><<<gn, 256, 0, st>>>(a); });
  // 2^bits > n_rows: a bad id's key keeps its low bits all set and sorts last
  int bits = 1;
  while (bits < 32 && ((uint64_t)1 << bits) <= (uint64_t)n_rows) ++bits;
  hipError_t e = sort_pairs_u32(a.key_in, a.val_in, a.key_out, a.val_out, a.n, bits, ws + w.sort, st);
  if (e != hipSuccess) {
    set_error("%s: radix sort failed: %s", what, hipGetErrorString(e));
    return RS_ERR_HIP;
  }
  fnn_heads_kernel<<<gn, 256, 0, st>>>(a);
  e = inclusive_sum_i32(a.scan, a.scan, a.n, ws + w.sort, st);
  if (e != hipSuccess) {
    set_error("%s: scan failed: %s", what, hipGetErrorString(e));
    return RS_ERR_HIP;
  }
  fnn_slots_kernel<<<gn, 256, 0, st>>>(a);
  const int64_t umax = std::min<int64_t>(a.n, n_rows);
  const unsigned gu = (unsigned)std::min<int64_t>((umax + 3) / 4, 1 << 14);
  const bool v4 = H1 % 4 == 0 && fnn_al16(W1) && fnn_al16(b1) && fnn_al16(out) && out_stride % 4 == 0 &&
                  fnn_al16(workspace);
  const unsigned gb = (unsigned)((batch + 3) / 4);
  if (v4) {
    fnn_pu_kernel<4><<<gu, 256, 0, st>>>(a);
    fnn_z1_kernel<4><<<gb, 256, 0, st>>>(a, b1, act, out, out_stride);
  } else {
    fnn_pu_kernel<1><<<gu, 256, 0, st>>>(a);
    fnn_z1_kernel<1><<<gb, 256, 0, st>>>(a, b1, act, out, out_stride);
  }
  return launch_status(what);
}

extern "C" int rs_fnn_w1_sgd(const float* d_a1, int64_t d_stride, const float* mult, int64_t mult_stride,
                             const float* mask, int64_t mask_stride, const float* dense, int64_t dense_stride,
                             int nd, int n_fields, const float* v, float* W1, int64_t n_rows, int k, int H1,
                             int64_t batch, float lr, float* dz1, float* g_out, void* workspace,
                             rs_stream_t stream) {
  if (batch == 0) return RS_OK;
  const char* what = "rs_fnn_w1_sgd";
  RS_REQUIRE(batch > 0 && nd >= 0 && n_fields >= 0 && nd + n_fields >= 1 && k >= 1 && H1 >= 1 && n_rows >= nd,
             "%s: bad shape", what);
  const int64_t n = batch * (nd + n_fields);
  RS_REQUIRE(n_rows < 0xffffffffll && n < (1ll << 31) && n * H1 < (1ll << 38),
             "%s: rows must fit uint32, lookups int32", what);
  RS_REQUIRE(d_a1 && d_stride >= H1 && (!mult || mult_stride >= H1) && (!mask || mask_stride >= H1) && v && dz1 &&
                 workspace && (nd == 0 || (dense && dense_stride >= nd)) && (W1 || g_out),
             "%s: null pointer or short stride", what);
  const FnnWs w = fnn_ws(batch, nd, n_fields, n_rows, H1);
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  FnnSgdArgs s{};
  s.t = FnnTrainArgs{nullptr, 0, dense, dense_stride, nd, nullptr, nullptr, n_fields, v, W1, n_rows, k, H1, batch, n,
                     reinterpret_cast<uint32_t*>(ws + w.key_in), reinterpret_cast<uint32_t*>(ws + w.key_out),
                     reinterpret_cast<uint32_t*>(ws + w.val_in), reinterpret_cast<uint32_t*>(ws + w.val_out),
                     reinterpret_cast<int32_t*>(ws + w.scan), reinterpret_cast<int32_t*>(ws + w.lslot),
                     reinterpret_cast<int32_t*>(ws + w.ustart), reinterpret_cast<float*>(ws + w.part),
                     reinterpret_cast<float*>(ws + w.pu), nullptr};
  s.dz1 = dz1;
  s.lr = lr;
  s.g_out = g_out;
  s.C = seg_chunk(H1);
  hipStream_t st = as_stream(stream);
  fnn_dz1_kernel<<<(unsigned)((batch * H1 + 255) / 256), 256, 0, st>>>(d_a1, d_stride, mult, mult_stride, mask,
                                                                        mask_stride, batch, H1, dz1);
  const unsigned g = (unsigned)((n * H1 + 255) / 256);
  fnn_piece_kernel<<<g, 256, 0, st>>>(s);
  if (n > s.C) fnn_cross_kernel<<<g, 256, 0, st>>>(s);
  return launch_status(what);
}
