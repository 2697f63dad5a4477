// fnn.hip — FNN inference (model/fnn.py:51-67): sigmoid(DNNLayer(x (.) v)) on
// the compact batch, without the dense [B, n*k] input.
//
// The reference multiplies the one-hot row x [n] into v [n, k], reshapes to
// [B, n*k] and feeds Dense(H1) with kernel W1 [n*k, H1].  x has A = nd + F
// non-zeros per sample (the nd dense features, one column per sparse field),
// so with W1 viewed as [n, k, H1]
//   z1[b, :] = b1 + sum_a x_a * (v[f_a, :] @ W1[f_a]) = b1 + sum_a x_a P[f_a]
// where P[f, :] = v[f, :] @ W1[f] ([n, H1]) depends on the weights only:
//   rs_fnn_project          P from (v, W1), one streaming pass over W1;
//   rs_fnn_first_layer_fwd  z1 (or act(z1)) [B, H1]: A rows of P per sample,
//                           one wave per sample, 16 B per lane per row;
//   rs_fnn_fwd              the same gather staged into the input tile of the
//                           fused tower (mlp_tower.hpp) for layers 2..L + the
//                           sigmoid head: a1 never reaches HBM.
// Sums run in a fixed order (dense features, then fields), so the two forward
// entries agree bit for bit on a1.  An out-of-range id sets RS_FLAG_BAD_ID
// and contributes a zero row.  Every offset into W1 / P is int64.
#include "mlp_tower.hpp"

namespace rs {

struct FnnIn {
  const void* ids;
  int64_t id_stride;
  const float* dense;
  int64_t ds;
  int nd;
  const int64_t* offs;  // one-hot field offsets (without nd)
  const int64_t* vocab;
  int F;
  const float* P;  // [n_rows, H1]
  int64_t n_rows;
  int H1;
  const float* b1;
  int act;
  int* err;
  int64_t B;
};

constexpr int FNN_U = 8;  // rows of P in flight per wave

// act-less z1 of sample m at columns c .. c+V-1 (c + V <= H1): b1, then the
// dense features in order, then the fields in order.
template <int KIND, int V>
__device__ __forceinline__ void fnn_gather(const FnnIn& a, int64_t m, int c, float (&acc)[V], bool& bad) {
  typedef Ids<KIND> I;
  Chunk<V> t;
  t.load(a.b1 + c);
#pragma unroll
  for (int q = 0; q < V; ++q) acc[q] = t.v[q];
  for (int j0 = 0; j0 < a.nd; j0 += FNN_U) {
    Chunk<V> p[FNN_U];
    float x[FNN_U];
#pragma unroll
    for (int u = 0; u < FNN_U; ++u) {
      const int j = j0 + u < a.nd ? j0 + u : a.nd - 1;
      x[u] = j0 + u < a.nd ? a.dense[m * a.ds + j] : 0.f;
      p[u].load_nt(a.P + (int64_t)j * a.H1 + c);
    }
#pragma unroll
    for (int u = 0; u < FNN_U; ++u)
      if (j0 + u < a.nd) {
#pragma unroll
        for (int q = 0; q < V; ++q) acc[q] = fmaf(x[u], p[u].v[q], acc[q]);
      }
  }
  for (int f0 = 0; f0 < a.F; f0 += FNN_U) {
    Chunk<V> p[FNN_U];
    bool ok[FNN_U];
#pragma unroll
    for (int u = 0; u < FNN_U; ++u) {
      const int f = f0 + u < a.F ? f0 + u : a.F - 1;
      int64_t id;
      ok[u] = I::decode(I::load(a.ids, m * a.id_stride + f), a.vocab[f], id);
      int64_t row = a.nd + a.offs[f] + id;
      if (row >= a.n_rows) {  // a layout that does not fit the table: as a bad id
        ok[u] = false;
        row = 0;
      }
      if (f0 + u < a.F) bad |= !ok[u];
      else ok[u] = false;
      p[u].load_nt(a.P + row * a.H1 + c);
    }
#pragma unroll
    for (int u = 0; u < FNN_U; ++u)
      if (ok[u]) {
#pragma unroll
        for (int q = 0; q < V; ++q) acc[q] += p[u].v[q];
      }
  }
}

template <int V>
__device__ __forceinline__ void fnn_store(float* dst, const float (&v)[V]) {
  if constexpr (V == 4) {
    floatx4 t = {v[0], v[1], v[2], v[3]};
    *reinterpret_cast<floatx4*>(dst) = t;
  } else {
    dst[0] = v[0];
  }
}

// One wave per sample; 64 V columns per pass.
template <int KIND, int V>
__global__ __launch_bounds__(256) void fnn_first_layer_kernel(FnnIn a, float* __restrict__ out, int64_t os) {
  const int lane = threadIdx.x & 63;
  const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= a.B) return;  // wave-uniform
  bool bad = false;
  for (int c = V * lane; c < a.H1; c += 64 * V) {
    float acc[V];
    fnn_gather<KIND, V>(a, m, c, acc, bad);
#pragma unroll
    for (int q = 0; q < V; ++q) acc[q] = mlp_act(acc[q], a.act, 0.f);
    fnn_store<V>(out + m * os + c, acc);
  }
  if (__any(bad) && lane == 0) flag_error(a.err);
}

// The one-launch forward: a 16-sample tile per workgroup, wave w gathers
// a1 of sample m0 + w into row w of the tower's input tile (rows past M
// re-read row M - 1 and are never stored; columns H1 .. Kp0-1 are zero), then
// the tower of layers 2..L and the head runs on the tile (mlp_tower_tile).
template <int NW, int KIND, int V>
__global__ __launch_bounds__(NW * 64) void fnn_fwd_kernel(MlpArgs a, FnnIn in) {
  extern __shared__ float smem[];
  const int RS = a.rs;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t m0 = (int64_t)blockIdx.x * 16;
  floatx4 ring[MLP_R];
  mlp_first_fill<NW>(a, ring);
  for (int r = w; r < 16; r += NW) {
    const bool live = m0 + r < a.M;
    const int64_t m = live ? m0 + r : a.M - 1;
    bool bad = false;
    for (int c = V * lane; c < a.Kp[0]; c += 64 * V) {
      float acc[V];
      if (c < in.H1) {
        fnn_gather<KIND, V>(in, m, c, acc, bad);
#pragma unroll
        for (int q = 0; q < V; ++q) acc[q] = mlp_act(acc[q], in.act, 0.f);
      } else {
#pragma unroll
        for (int q = 0; q < V; ++q) acc[q] = 0.f;
      }
      fnn_store<V>(smem + r * RS + c, acc);
    }
    if (__any(bad && live) && lane == 0) flag_error(in.err);
  }
  float* par = smem + 32 * RS + NW * 256;
  for (int i = threadIdx.x; i < a.ptot; i += NW * 64) par[i] = a.prep[a.wtot + i];
  mlp_tower_tile<NW>(a, smem, m0, ring);
}

// P[f, c] = sum_j v[f, j] W1[(f k + j) H1 + c], j in order (fmaf chain): one
// thread per V columns of one row, W1 streamed once (non-temporal).
template <int V>
__global__ __launch_bounds__(256) void fnn_project_kernel(const float* __restrict__ v, const float* __restrict__ W1,
                                                          int64_t n_rows, int k, int H1, float* __restrict__ P) {
  const int cv = H1 / V;
  const int64_t total = n_rows * cv;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    const int64_t f = t / cv;
    const int c = (int)(t - f * cv) * V;
    float acc[V];
#pragma unroll
    for (int q = 0; q < V; ++q) acc[q] = 0.f;
    const float* wr = W1 + f * k * (int64_t)H1 + c;
    for (int j0 = 0; j0 < k; j0 += 4) {
      Chunk<V> w[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) w[u].load_nt(wr + (int64_t)(j0 + u < k ? j0 + u : k - 1) * H1);
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (j0 + u < k) {
          const float vj = v[f * k + j0 + u];
#pragma unroll
          for (int q = 0; q < V; ++q) acc[q] = fmaf(vj, w[u].v[q], acc[q]);
        }
    }
    fnn_store<V>(P + f * H1 + c, acc);
  }
}

static bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static bool fnn_act_ok(int act) { return act == RS_ACT_NONE || act == RS_ACT_RELU || act == RS_ACT_SIGMOID; }

// n_layers Dense layers (the gathered first one included) of output widths
// dims[0 .. n_layers-1], dims[n_layers-1] == 1: the tower part's geometry
static bool fnn_geom(int n_layers, const int* dims, const int* acts, MlpGeom& g) {
  if (n_layers < 2 || n_layers > MLP_MAXL + 1 || !dims || !acts) return false;
  for (int l = 0; l < n_layers; ++l)
    if (!fnn_act_ok(acts[l])) return false;
  if (dims[n_layers - 1] != 1) return false;
  return mlp_geom(n_layers - 1, dims, g);
}

static int fnn_fill(const char* what, const void* ids, int id_kind, int64_t id_stride, const float* dense,
                    int64_t dense_stride, int nd, const int64_t* field_offsets, const int64_t* field_vocab,
                    int n_fields, const float* P, int64_t n_rows, int H1, const float* b1, int act, int64_t batch,
                    int* err_flag, FnnIn& in) {
  RS_REQUIRE(batch > 0 && nd >= 0 && n_fields >= 0 && nd + n_fields >= 1 && H1 >= 1 && n_rows >= nd,
             "%s: bad shape", what);
  RS_REQUIRE(P && b1 && (nd == 0 || (dense && dense_stride >= nd)) &&
                 (n_fields == 0 || (ids && field_offsets && field_vocab && id_stride >= n_fields && err_flag)),
             "%s: null pointer or short stride", what);
  RS_REQUIRE(id_kind >= RS_ID_I32 && id_kind <= RS_ID_F32, "%s: bad id_kind", what);
  RS_REQUIRE(fnn_act_ok(act), "%s: the first layer's activation must be none, relu or sigmoid", what);
  in = FnnIn{ids, id_stride, dense, dense_stride, nd, field_offsets, field_vocab, n_fields, P, n_rows, H1, b1, act,
             err_flag, batch};
  return RS_OK;
}

}  // namespace rs

using namespace rs;

extern "C" int rs_fnn_project(const float* v, const float* W1, int64_t n_rows, int k, int H1, float* P,
                              rs_stream_t stream) {
  if (n_rows == 0) return RS_OK;
  RS_REQUIRE(v && W1 && P && n_rows > 0 && k >= 1 && H1 >= 1, "rs_fnn_project: bad arguments");
  hipStream_t st = as_stream(stream);
  const bool v4 = H1 % 4 == 0 && al16(W1) && al16(P);
  const int64_t total = n_rows * (v4 ? H1 / 4 : H1);
  const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, 1 << 16);
  if (v4) fnn_project_kernel<4><<<grid, 256, 0, st>>>(v, W1, n_rows, k, H1, P);
  else fnn_project_kernel<1><<<grid, 256, 0, st>>>(v, W1, n_rows, k, H1, P);
  return launch_status("rs_fnn_project");
}

extern "C" int rs_fnn_first_layer_fwd(const void* ids, int id_kind, int64_t id_stride, const float* dense,
                                      int64_t dense_stride, int nd, const int64_t* field_offsets,
                                      const int64_t* field_vocab, int n_fields, const float* P, int64_t n_rows,
                                      int H1, const float* b1, int act, float* out, int64_t out_stride,
                                      int64_t batch, int* err_flag, rs_stream_t stream) {
  if (batch == 0) return RS_OK;
  const char* what = "rs_fnn_first_layer_fwd";
  FnnIn in;
  const int s = fnn_fill(what, ids, id_kind, id_stride, dense, dense_stride, nd, field_offsets, field_vocab,
                         n_fields, P, n_rows, H1, b1, act, batch, err_flag, in);
  if (s != RS_OK) return s;
  RS_REQUIRE(out && out_stride >= H1, "%s: null or short output", what);
  RS_REQUIRE((batch + 3) / 4 < (1ll << 31), "%s: batch too large", what);
  const bool v4 = H1 % 4 == 0 && al16(P) && al16(b1) && al16(out) && out_stride % 4 == 0;
  const unsigned grid = (unsigned)((batch + 3) / 4);
  hipStream_t st = as_stream(stream);
  with_id_kind(id_kind, [&](auto K) {
    constexpr int KD = decltype(K)::value;
    if (v4) fnn_first_layer_kernel<KD, 4><<<grid, 256, 0, st>>>(in, out, out_stride);
    else fnn_first_layer_kernel<KD, 1><<<grid, 256, 0, st>>>(in, out, out_stride);
  });
  return launch_status(what);
}

extern "C" int rs_fnn_ok(int n_layers, const int* dims, const int* acts) {
  MlpGeom g;
  return fnn_geom(n_layers, dims, acts, g) ? 1 : 0;
}

extern "C" int rs_fnn_fwd(const void* ids, int id_kind, int64_t id_stride, const float* dense, int64_t dense_stride,
                          int nd, const int64_t* field_offsets, const int64_t* field_vocab, int n_fields,
                          const float* P, int64_t n_rows, const float* b1, int n_layers, const int* dims,
                          const int* acts, const float* prepared, float* y, int64_t y_stride, int64_t batch,
                          int* err_flag, rs_stream_t stream) {
  if (batch == 0) return RS_OK;
  const char* what = "rs_fnn_fwd";
  MlpGeom g;
  RS_REQUIRE(fnn_geom(n_layers, dims, acts, g),
             "%s: shape not supported (rs_fnn_ok: 2..%d layers of widths 1..%d ending in 1, none / relu / sigmoid, "
             "the tile's LDS <= 160 KiB)",
             what, MLP_MAXL + 1, MLP_MAXD);
  FnnIn in;
  const int s = fnn_fill(what, ids, id_kind, id_stride, dense, dense_stride, nd, field_offsets, field_vocab,
                         n_fields, P, n_rows, dims[0], b1, acts[0], batch, err_flag, in);
  if (s != RS_OK) return s;
  RS_REQUIRE(prepared && y && y_stride >= 1, "%s: null pointer", what);
  MlpArgs a{};
  RS_REQUIRE(mlp_fill_args(g, acts + 1, prepared, a), "%s: bad activation", what);
  a.y = y;
  a.ys = y_stride;
  a.head = 1;  // sigmoid(1 * z)
  a.c0 = 1.f;
  a.c1 = 0.f;
  a.M = batch;
  const int64_t grid = (batch + 15) / 16;
  RS_REQUIRE(grid < (1ll << 31), "%s: batch too large", what);
  const bool v4 = in.H1 % 4 == 0 && al16(P) && al16(b1);
  hipStream_t st = as_stream(stream);
  with_id_kind(id_kind, [&](auto K) {
    constexpr int KD = decltype(K)::value;
    if (v4) launch_lds<fnn_fwd_kernel<MLP_NW, KD, 4>>((unsigned)grid, MLP_NW * 64, g.lds, st, a, in);
    else launch_lds<fnn_fwd_kernel<MLP_NW, KD, 1>>((unsigned)grid, MLP_NW * 64, g.lds, st, a, in);
  });
  return launch_status(what);
}
