// fgcnn.hip — the convolution stack of FGCNNLayer (layer/interaction.py:218-258):
// per layer Conv2D(filters, (kernel_width, 1), 'same', tanh) along the field
// axis, then MaxPool2D((pooling_width, 1)), for a tile of samples in ONE
// launch.  The recombination Dense of each layer is rs_dense_fwd on the
// workspace this kernel fills.
//
// Per sample the zero-padded input map of every layer lives in LDS, flat as
// [h][d][c] (h: field row incl. the 'same' padding, d: embedding column, c:
// channel).  A layer's convolution is a GEMM per sample: M = the pooled
// positions mp = h' k + d, K = (t, c) = kw Cin taps, N = Cout.  Row mp of pool
// member j reads A[mp][(t,c)] = x[((h' pw + j + t) k + d) Cin + c] — the im2col
// is addressing only — and B is the Keras kernel [kw, 1, Cin, Cout] as it is
// ([(t,c)][n], staged in LDS once per workgroup).  One wave owns a 16-row
// M tile and both 16-column N tiles (Cout <= 32) as v_mfma_f32_16x16x4_f32
// chains; the pw pool members are folded with max in registers BEFORE bias +
// tanh (tanh is monotonic, so max(tanh(x_j + b)) = tanh(max(x_j) + b)), which
// also spares pw - 1 of every pw tanhf calls.  The pooled value goes to the
// next layer's padded map in LDS and to the workspace row in Keras Flatten
// order [h'][d][n] = mp Cout + n.
#include "rs_common.hpp"

namespace rs {

constexpr int FG_MAXL = 4;
constexpr int FG_NT = 256, FG_NW = FG_NT / 64;
constexpr int FG_SMAX = 4;                 // samples per workgroup
constexpr int64_t FG_LDS_MAX = 128 * 1024;  // bytes, weights + one sample at least

struct FgLayer {
  const float* w;  // [kw, 1, Cin, Cout]
  const float* b;  // [Cout]
  int H, Hp, Cin, Cout, kw, pw;
  int in_off;   // the padded input map [H + kw - 1][k][Cin], floats from the sample's base
  int w_off;    // weights then bias, floats from the LDS base
  int ws_off;   // first workspace column of this layer's pooled map
};

struct FgArgs {
  const float* emb;  // [B, F, k] (when ids == nullptr)
  const void* ids;
  int64_t id_stride;
  const float* table;
  const int64_t* offs;
  const int64_t* vocab;
  int F, k, L, S;
  int wtot;  // floats of staged weights (the samples' maps start there)
  int per;   // floats per sample
  float* ws;
  int64_t ws_stride;
  float* z;  // ids form: the gathered rows also go to z[b, 0:F*k] (may be null)
  int64_t z_stride;
  int64_t batch;
  int* err;
  FgLayer l[FG_MAXL];
};

template <int KIND>
__global__ __launch_bounds__(FG_NT) void fgcnn_conv(FgArgs a) {
  typedef Ids<KIND == 3 ? 0 : KIND> I;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int k = a.k, S = a.S;
  const int64_t b0 = (int64_t)blockIdx.x * S;
  const int nvalid = (int)(a.batch - b0 < S ? a.batch - b0 : S);
  float* maps = smem + a.wtot;

  // weights + biases -> LDS; the maps zeroed (the 'same' padding rows stay 0)
  for (int li = 0; li < a.L; ++li) {
    const FgLayer& l = a.l[li];
    const int nw = l.kw * l.Cin * l.Cout;
    for (int i = tid; i < nw; i += FG_NT) smem[l.w_off + i] = l.w[i];
    for (int i = tid; i < l.Cout; i += FG_NT) smem[l.w_off + nw + i] = l.b[i];
  }
  for (int i = tid; i < S * a.per / 4; i += FG_NT)
    reinterpret_cast<floatx4*>(maps)[i] = floatx4{0.f, 0.f, 0.f, 0.f};
  __syncthreads();

  // layer 0 input: the F rows of every sample (gathered, or given)
  {
    const int KQ = k / 4, per_s = a.F * KQ;
    const int pb = (a.l[0].kw - 1) / 2;
    bool bad = false;
    for (int i = tid; i < nvalid * per_s; i += FG_NT) {
      const int s = i / per_s, r = i - s * per_s;
      const int c = r / KQ, q = r - c * KQ;
      const int64_t b = b0 + s;
      floatx4 v = {0.f, 0.f, 0.f, 0.f};
      if constexpr (KIND == 3) {
        v = __builtin_nontemporal_load(reinterpret_cast<const floatx4*>(a.emb + (b * a.F + c) * k + 4 * q));
      } else {
        int64_t id;
        const bool ok = I::decode(I::load(a.ids, b * a.id_stride + c), a.vocab[c], id);
        const floatx4 t = *reinterpret_cast<const floatx4*>(a.table + (a.offs[c] + id) * k + 4 * q);
        if (ok) v = t;
        bad |= !ok;
        if (a.z) *reinterpret_cast<floatx4*>(a.z + b * a.z_stride + c * k + 4 * q) = v;
      }
      *reinterpret_cast<floatx4*>(maps + s * a.per + a.l[0].in_off + (pb + c) * k + 4 * q) = v;
    }
    if (bad) flag_error(a.err);
  }
  __syncthreads();

  const int rowl = lane & 15, kq = lane >> 4;
  for (int li = 0; li < a.L; ++li) {
    const FgLayer& l = a.l[li];
    const int Cin = l.Cin, Cout = l.Cout, pw = l.pw;
    const int Mp = l.Hp * k, MT = (Mp + 15) >> 4, K = l.kw * Cin;
    const bool two = Cout > 16;
    const float* wl = smem + l.w_off;
    const float* bl = wl + K * Cout;
    const bool last = li + 1 == a.L;
    const int nx_off = last ? 0 : a.l[li + 1].in_off + ((a.l[li + 1].kw - 1) / 2) * k * Cout;
    for (int task = w; task < nvalid * MT; task += FG_NW) {
      const int s = task / MT, mt = task - s * MT;
      const float* x = maps + s * a.per + l.in_off;
      // this lane's A row: pooled position mp = (h', d); rows past Mp read row 0 (discarded)
      int mp = 16 * mt + rowl;
      mp = mp < Mp ? mp : 0;
      const int hp = mp / k, d = mp - hp * k;
      const int n0 = rowl, n1 = 16 + rowl;
      floatx4 mx0, mx1;
      for (int j = 0; j < pw; ++j) {
        const int abase = ((hp * pw + j) * k + d) * Cin;
        floatx4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = c0;
        int t = 0, c = kq;  // tap kk = t Cin + c, advanced by 4 per step (no division in the loop)
        while (c >= Cin) {
          c -= Cin;
          ++t;
        }
        for (int kk0 = 0; kk0 < K; kk0 += 4) {
          const int kk = kk0 + kq;
          const bool kin = kk < K;
          const int kc = kin ? kk : 0;
          const float av = x[abase + (kin ? t * k * Cin + c : 0)];
          const float am = kin ? av : 0.f;
          c += 4;
          while (c >= Cin) {
            c -= Cin;
            ++t;
          }
          const float bv0 = wl[kc * Cout + (n0 < Cout ? n0 : 0)];
          c0 = mfma16x16x4(am, (kin && n0 < Cout) ? bv0 : 0.f, c0);
          if (two) {
            const float bv1 = wl[kc * Cout + (n1 < Cout ? n1 : 0)];
            c1 = mfma16x16x4(am, (kin && n1 < Cout) ? bv1 : 0.f, c1);
          }
        }
        if (j == 0) {
          mx0 = c0;
          mx1 = c1;
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            mx0[r] = fmaxf(mx0[r], c0[r]);
            mx1[r] = fmaxf(mx1[r], c1[r]);
          }
        }
      }
      // C[row = 4 kq + r][col = rowl]: bias + tanh, to the next map and the workspace
      float* wsr = a.ws + (b0 + s) * a.ws_stride + l.ws_off;
      float* nx = maps + s * a.per + nx_off;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = 16 * mt + 4 * kq + r;
        if (m >= Mp) continue;
        if (n0 < Cout) {
          const float v = tanhf(mx0[r] + bl[n0]);
          wsr[m * Cout + n0] = v;
          if (!last) nx[m * Cout + n0] = v;
        }
        if (two && n1 < Cout) {
          const float v = tanhf(mx1[r] + bl[n1]);
          wsr[m * Cout + n1] = v;
          if (!last) nx[m * Cout + n1] = v;
        }
      }
    }
    if (!last) __syncthreads();
  }
}

// Shapes of the stack for n_fields x k: fills the layers (H, Hp, Cin, LDS and
// workspace offsets) and returns the workspace floats per sample, or -1 with
// the error string set.
static int64_t fg_plan(const char* what, int F, int k, int L, const int* filters, const int* kw, const int* pw,
                       FgArgs* a) {
  if (!(L >= 1 && L <= FG_MAXL)) {
    set_error("%s: need 1..%d conv layers", what, FG_MAXL);
    return -1;
  }
  if (!filters || !kw || !pw) {
    set_error("%s: null pointer", what);
    return -1;
  }
  if (!(k == 4 || k == 8 || k == 16 || k == 32 || k == 64) || F < 1) {
    set_error("%s: need >= 1 field and k in {4,8,16,32,64}", what);
    return -1;
  }
  int64_t H = F, Cin = 1, ws = 0, per = 0, wtot = 0;
  for (int i = 0; i < L; ++i) {
    if (!(filters[i] >= 1 && filters[i] <= 32 && kw[i] >= 1 && pw[i] >= 1)) {
      set_error("%s: layer %d needs 1..32 filters, kernel_width >= 1, pooling_width >= 1", what, i);
      return -1;
    }
    const int64_t Hp = H / pw[i];
    if (Hp < 1) {
      set_error("%s: layer %d pools %lld rows by %d: nothing left", what, i, (long long)H, pw[i]);
      return -1;
    }
    const int64_t map = (H + kw[i] - 1) * k * Cin;            // a multiple of 4 (k is)
    const int64_t wn = ((int64_t)kw[i] * Cin * filters[i] + filters[i] + 3) / 4 * 4;
    if ((wtot + wn + per + map) * 4 > FG_LDS_MAX) {
      set_error("%s: the per-sample LDS tile does not fit (layer %d)", what, i);
      return -1;
    }
    if (a) {
      FgLayer& l = a->l[i];
      l.H = (int)H;
      l.Hp = (int)Hp;
      l.Cin = (int)Cin;
      l.Cout = filters[i];
      l.kw = kw[i];
      l.pw = pw[i];
      l.in_off = (int)per;
      l.w_off = (int)wtot;
      l.ws_off = (int)ws;
    }
    per += map;
    wtot += wn;
    ws += Hp * k * filters[i];
    H = Hp;
    Cin = filters[i];
  }
  if (a) {
    a->per = (int)per;
    a->wtot = (int)wtot;
  }
  return ws;
}

static int fg_launch(const char* what, FgArgs& a, int id_kind, const int* filters, const int* kw, const int* pw,
                     const float* const* conv_w, const float* const* conv_b, hipStream_t st) {
  const int64_t need = fg_plan(what, a.F, a.k, a.L, filters, kw, pw, &a);
  if (need < 0) return RS_ERR_ARG;
  RS_REQUIRE(conv_w && conv_b && a.ws, "%s: null pointer", what);
  RS_REQUIRE(a.ws_stride >= need, "%s: workspace stride %lld < %lld", what, (long long)a.ws_stride, (long long)need);
  for (int i = 0; i < a.L; ++i) {
    RS_REQUIRE(conv_w[i] && conv_b[i], "%s: null weights (layer %d)", what, i);
    a.l[i].w = conv_w[i];
    a.l[i].b = conv_b[i];
  }
  int S = FG_SMAX;
  while (S > 1 && ((int64_t)a.wtot + (int64_t)S * a.per) * 4 > 64 * 1024) --S;
  a.S = S;
  const size_t lds = ((size_t)a.wtot + (size_t)S * a.per) * sizeof(float);
  const unsigned grid = (unsigned)((a.batch + S - 1) / S);
  if (a.ids == nullptr) launch_lds<fgcnn_conv<3>>(grid, FG_NT, lds, st, a);
  else with_id_kind(id_kind, [&](auto KI) { launch_lds<fgcnn_conv<decltype(KI)::value>>(grid, FG_NT, lds, st, a); });
  return launch_status(what);
}

}  // namespace rs

using namespace rs;

extern "C" int64_t rs_fgcnn_workspace_size(int n_fields, int k, int n_layers, const int* filters,
                                           const int* kernel_width, const int* pooling_width) {
  return fg_plan("rs_fgcnn_workspace_size", n_fields, k, n_layers, filters, kernel_width, pooling_width, nullptr);
}

extern "C" int rs_fgcnn_conv_fwd(const float* emb, int n_fields, int k, int n_layers, const int* filters,
                                 const int* kernel_width, const int* pooling_width, const float* const* conv_w,
                                 const float* const* conv_b, float* workspace, int64_t ws_stride, int64_t batch,
                                 rs_stream_t stream) {
  if (batch == 0) return RS_OK;  // empty batch: nothing to launch (null data pointers allowed)
  RS_REQUIRE(batch >= 0, "rs_fgcnn_conv_fwd: negative batch");
  RS_REQUIRE(emb && workspace, "rs_fgcnn_conv_fwd: null pointer");
  RS_REQUIRE((uintptr_t)emb % 16 == 0, "rs_fgcnn_conv_fwd: emb must be 16-B aligned");
  FgArgs a{};
  a.emb = emb;
  a.F = n_fields;
  a.k = k;
  a.L = n_layers;
  a.ws = workspace;
  a.ws_stride = ws_stride;
  a.batch = batch;
  return fg_launch("rs_fgcnn_conv_fwd", a, 0, filters, kernel_width, pooling_width, conv_w, conv_b,
                   as_stream(stream));
}

extern "C" int rs_embed_fgcnn_conv_fwd(const void* ids, int id_kind, int64_t id_stride, const float* table,
                                       const int64_t* field_offsets, const int64_t* field_vocab, int n_fields, int k,
                                       int n_layers, const int* filters, const int* kernel_width,
                                       const int* pooling_width, const float* const* conv_w,
                                       const float* const* conv_b, float* workspace, int64_t ws_stride, float* z,
                                       int64_t z_stride, int64_t batch, int* err_flag, rs_stream_t stream) {
  if (batch == 0) return RS_OK;  // empty batch: nothing to launch (null data pointers allowed)
  RS_REQUIRE(batch >= 0, "rs_embed_fgcnn_conv_fwd: negative batch");
  RS_REQUIRE(ids && table && field_offsets && field_vocab && workspace, "rs_embed_fgcnn_conv_fwd: null pointer");
  RS_REQUIRE(id_kind >= RS_ID_I32 && id_kind <= RS_ID_F32, "rs_embed_fgcnn_conv_fwd: bad id_kind");
  RS_REQUIRE((uintptr_t)table % 16 == 0, "rs_embed_fgcnn_conv_fwd: table must be 16-B aligned");
  RS_REQUIRE(!z || ((uintptr_t)z % 16 == 0 && z_stride % 4 == 0 && z_stride >= (int64_t)n_fields * k),
             "rs_embed_fgcnn_conv_fwd: z must be 16-B aligned, its stride a multiple of 4 and >= F*k");
  FgArgs a{};
  a.ids = ids;
  a.id_stride = id_stride;
  a.table = table;
  a.offs = field_offsets;
  a.vocab = field_vocab;
  a.F = n_fields;
  a.k = k;
  a.L = n_layers;
  a.ws = workspace;
  a.ws_stride = ws_stride;
  a.z = z;
  a.z_stride = z_stride;
  a.batch = batch;
  a.err = err_flag;
  return fg_launch("rs_embed_fgcnn_conv_fwd", a, id_kind, filters, kernel_width, pooling_width, conv_w, conv_b,
                   as_stream(stream));
}
