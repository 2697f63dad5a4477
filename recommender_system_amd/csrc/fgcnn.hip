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

// ------------------------------------------------------------------ backward
// The whole stack's backward in ONE launch (rs_fgcnn_conv_bwd).  A workgroup
// takes samples b = blockIdx.x, + gridDim.x, ... one at a time and walks the
// layers top down with four LDS regions: the layer's kernel, its zero-padded
// input map X [H + kw - 1][k][Cin] (the rows for layer 0, the saved pooled map
// of the layer below otherwise), its zero-padded gradient map dY
// [H + kw - 1][k][Cout] (kw - 1 - pb rows in front, pb behind: the transposed
// convolution's 'same' padding) and G [Hp][k][Cout], which carries a layer's
// input gradient down to the next layer's pooled gradient.  Per layer:
//   1. one thread per pooled value recomputes the pw members' conv sums (fp32
//      chains in (t, c) order; the bias is common to the members), routes
//      (dws + G) (1 - p^2) to the FIRST member that attains the maximum — p is
//      the saved tanh(max + b) — and leaves every other dY entry zero;
//   2. db[n] = sum dY, dW[t,c,n] = sum_{h,d} X[h+t,d,c] dY[h,d,n]: one thread
//      per element, added into the workgroup's own partial row (the same
//      thread owns the element for every sample: no atomics);
//   3. dX[h,d,c] = sum_{t,n} dY[h - t + pb,d,n] W[t,c,n] into G, or for layer 0
//      added into the caller's de.
// fgcnn_bwd_finish then sums the partial rows in a fixed order.
constexpr int FG_BWD_GRID = 512;  // workgroups (= partial rows) at most

struct FgBwdArgs {
  const float* z;
  int64_t z_stride;
  const float* ws;
  int64_t ws_stride;
  const float* dws;
  int64_t dws_stride;
  float* de;
  int64_t de_stride;
  float* part;  // [gridDim.x][gtot]: per layer dW then db
  int k, L;
  int xoff, yoff, goff;  // LDS regions after the kernel, floats
  int gtot;
  int64_t batch;
  FgLayer l[FG_MAXL];
  int g_off[FG_MAXL];  // the layer's first column of a partial row
};

__global__ __launch_bounds__(FG_NT) void fgcnn_conv_bwd(FgBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* wl = smem;
  float* X = smem + a.xoff;
  float* dY = smem + a.yoff;
  float* G = smem + a.goff;
  const int tid = threadIdx.x, k = a.k;
  float* part = a.part + (int64_t)blockIdx.x * a.gtot;
  bool first = true;
  for (int64_t b = blockIdx.x; b < a.batch; b += gridDim.x, first = false) {
    for (int li = a.L - 1; li >= 0; --li) {
      const FgLayer& l = a.l[li];
      const int Cin = l.Cin, Cout = l.Cout, kw = l.kw, pw = l.pw, H = l.H;
      const int pb = (kw - 1) / 2, pf = kw - 1 - pb, HP = H + kw - 1;
      const int nw = kw * Cin * Cout, nin = H * k * Cin, np = l.Hp * k * Cout;
      __syncthreads();  // the layer above is done with wl, X and dY
      for (int i = tid; i < nw; i += FG_NT) wl[i] = l.w[i];
      for (int i = tid; i < HP * k * Cin; i += FG_NT) X[i] = 0.f;
      for (int i = tid; i < HP * k * Cout; i += FG_NT) dY[i] = 0.f;
      __syncthreads();
      const float* src = li == 0 ? a.z + b * a.z_stride : a.ws + b * a.ws_stride + a.l[li - 1].ws_off;
      for (int i = tid; i < nin; i += FG_NT) X[pb * k * Cin + i] = src[i];
      __syncthreads();
      // 1. the pool's winner takes the gradient
      const float* pv = a.ws + b * a.ws_stride + l.ws_off;
      const float* dv = a.dws + b * a.dws_stride + l.ws_off;
      const bool top = li + 1 == a.L;
      for (int i = tid; i < np; i += FG_NT) {
        const int n = i % Cout, m = i / Cout, d = m % k, hp = m / k;
        float best = 0.f;
        int jb = 0;
        for (int j = 0; j < pw; ++j) {
          const float* xr = X + ((hp * pw + j) * k + d) * Cin;
          float acc = 0.f;
          for (int t = 0; t < kw; ++t)
            for (int c = 0; c < Cin; ++c) acc = fmaf(xr[t * k * Cin + c], wl[(t * Cin + c) * Cout + n], acc);
          if (j == 0 || acc > best) {
            best = acc;
            jb = j;
          }
        }
        float g = dv[i];
        if (!top) g += G[i];
        const float p = pv[i];
        dY[((pf + hp * pw + jb) * k + d) * Cout + n] = g * (1.f - p * p);
      }
      __syncthreads();
      // 2. bias and kernel gradients into this workgroup's partial row
      float* pr = part + a.g_off[li];
      for (int n = tid; n < Cout; n += FG_NT) {
        float s = 0.f;
        for (int r = 0; r < H * k; ++r) s += dY[(pf * k + r) * Cout + n];
        pr[nw + n] = first ? s : pr[nw + n] + s;
      }
      for (int e = tid; e < nw; e += FG_NT) {
        const int n = e % Cout, tc = e / Cout, c = tc % Cin, t = tc / Cin;
        const float* xr = X + t * k * Cin + c;
        const float* yr = dY + pf * k * Cout + n;
        float s = 0.f;
        for (int r = 0; r < H * k; ++r) s = fmaf(xr[r * Cin], yr[r * Cout], s);
        pr[e] = first ? s : pr[e] + s;
      }
      // 3. the transposed convolution
      for (int i = tid; i < nin; i += FG_NT) {
        const int c = i % Cin, m = i / Cin, d = m % k, h = m / k;
        float s = 0.f;
        for (int t = 0; t < kw; ++t) {
          const float* yr = dY + ((h + kw - 1 - t) * k + d) * Cout;
          const float* wr = wl + (t * Cin + c) * Cout;
          for (int n = 0; n < Cout; ++n) s = fmaf(yr[n], wr[n], s);
        }
        if (li == 0) a.de[b * a.de_stride + i] += s;
        else G[i] = s;
      }
    }
  }
}

struct FgFinish {
  float* dw[FG_MAXL];
  float* db[FG_MAXL];
  int g_off[FG_MAXL + 1];
  int nw[FG_MAXL];
  int L;
};

// column c of the partial rows summed in row order, four interleaved chains
__global__ __launch_bounds__(256) void fgcnn_bwd_finish(const float* __restrict__ part, int rows, int gtot,
                                                        FgFinish f) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= gtot) return;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  for (int r = 0; r < rows; ++r) s[r & 3] += part[(int64_t)r * gtot + c];
  const float v = (s[0] + s[1]) + (s[2] + s[3]);
  int li = 0;
  while (li + 1 < f.L && c >= f.g_off[li + 1]) ++li;
  const int e = c - f.g_off[li];
  if (e < f.nw[li]) f.dw[li][e] = v;
  else f.db[li][e - f.nw[li]] = v;
}

// The backward's plan on top of fg_plan: LDS regions and the partial row's
// layout.  Returns the LDS bytes, or -1 with the error string set.
static int64_t fg_bwd_plan(const char* what, int F, int k, int L, const int* filters, const int* kw, const int* pw,
                           FgBwdArgs* a) {
  FgArgs fa{};
  if (fg_plan(what, F, k, L, filters, kw, pw, &fa) < 0) return -1;
  int64_t wmax = 0, xmax = 0, ymax = 0, gmax = 0, gtot = 0;
  for (int i = 0; i < L; ++i) {
    const FgLayer& l = fa.l[i];
    const int64_t hp = l.H + l.kw - 1, nw = (int64_t)l.kw * l.Cin * l.Cout;
    wmax = std::max(wmax, (nw + 3) / 4 * 4);
    xmax = std::max(xmax, hp * k * l.Cin);
    ymax = std::max(ymax, hp * k * l.Cout);
    gmax = std::max(gmax, (int64_t)l.Hp * k * l.Cout);
    a->l[i] = l;
    a->g_off[i] = (int)gtot;
    gtot += nw + l.Cout;
  }
  const int64_t lds = (wmax + xmax + ymax + gmax) * 4;
  if (lds > FG_LDS_MAX) {
    set_error("%s: the backward's per-sample LDS tile does not fit (%lld > %lld bytes)", what, (long long)lds,
              (long long)FG_LDS_MAX);
    return -1;
  }
  a->k = k;
  a->L = L;
  a->xoff = (int)wmax;
  a->yoff = (int)(wmax + xmax);
  a->goff = (int)(wmax + xmax + ymax);
  a->gtot = (int)gtot;
  return lds;
}

}  // namespace rs

using namespace rs;

extern "C" int64_t rs_fgcnn_conv_bwd_workspace_size(int n_fields, int k, int n_layers, const int* filters,
                                                    const int* kernel_width, const int* pooling_width,
                                                    int64_t batch) {
  FgBwdArgs a{};
  if (batch < 0) {
    set_error("rs_fgcnn_conv_bwd_workspace_size: negative batch");
    return -1;
  }
  if (fg_bwd_plan("rs_fgcnn_conv_bwd_workspace_size", n_fields, k, n_layers, filters, kernel_width, pooling_width,
                  &a) < 0)
    return -1;
  return std::min<int64_t>(batch, FG_BWD_GRID) * a.gtot * 4;
}

extern "C" int rs_fgcnn_conv_bwd(const float* z, int64_t z_stride, const float* ws, int64_t ws_stride,
                                 const float* dws, int64_t dws_stride, int n_fields, int k, int n_layers,
                                 const int* filters, const int* kernel_width, const int* pooling_width,
                                 const float* const* conv_w, float* de, int64_t de_stride, float* const* dconv_w,
                                 float* const* dconv_b, void* workspace, int64_t workspace_bytes, int64_t batch,
                                 rs_stream_t stream) {
  if (batch == 0) return RS_OK;  // empty batch: nothing to launch (null data pointers allowed)
  RS_REQUIRE(batch > 0, "rs_fgcnn_conv_bwd: negative batch");
  RS_REQUIRE(z && ws && dws && de && conv_w && dconv_w && dconv_b && workspace, "rs_fgcnn_conv_bwd: null pointer");
  FgBwdArgs a{};
  const int64_t lds = fg_bwd_plan("rs_fgcnn_conv_bwd", n_fields, k, n_layers, filters, kernel_width, pooling_width, &a);
  if (lds < 0) return RS_ERR_ARG;
  const int64_t fk = (int64_t)n_fields * k, need = a.l[a.L - 1].ws_off + (int64_t)a.l[a.L - 1].Hp * k * a.l[a.L - 1].Cout;
  RS_REQUIRE(z_stride >= fk && de_stride >= fk, "rs_fgcnn_conv_bwd: z / de stride < F*k");
  RS_REQUIRE(ws_stride >= need && dws_stride >= need, "rs_fgcnn_conv_bwd: workspace stride < %lld", (long long)need);
  const int64_t grid = std::min<int64_t>(batch, FG_BWD_GRID);
  RS_REQUIRE(workspace_bytes >= grid * a.gtot * 4, "rs_fgcnn_conv_bwd: workspace of %lld bytes < %lld",
             (long long)workspace_bytes, (long long)(grid * a.gtot * 4));
  FgFinish f{};
  f.L = a.L;
  for (int i = 0; i < a.L; ++i) {
    RS_REQUIRE(conv_w[i] && dconv_w[i] && dconv_b[i], "rs_fgcnn_conv_bwd: null weights (layer %d)", i);
    a.l[i].w = conv_w[i];
    f.dw[i] = dconv_w[i];
    f.db[i] = dconv_b[i];
    f.g_off[i] = a.g_off[i];
    f.nw[i] = a.l[i].kw * a.l[i].Cin * a.l[i].Cout;
  }
  f.g_off[a.L] = a.gtot;
  a.z = z;
  a.z_stride = z_stride;
  a.ws = ws;
  a.ws_stride = ws_stride;
  a.dws = dws;
  a.dws_stride = dws_stride;
  a.de = de;
  a.de_stride = de_stride;
  a.part = static_cast<float*>(workspace);
  a.batch = batch;
  hipStream_t st = as_stream(stream);
  launch_lds<fgcnn_conv_bwd>((unsigned)grid, FG_NT, (size_t)lds, st, a);
  fgcnn_bwd_finish<<<(unsigned)((a.gtot + 255) / 256), 256, 0, st>>>(a.part, (int)grid, a.gtot, f);
  return launch_status("rs_fgcnn_conv_bwd");
}

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
