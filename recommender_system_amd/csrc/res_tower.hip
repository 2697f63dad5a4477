// res_tower.hip — DeepCrossing's stack of residual units in one launch:
// ResLayer (layer/interaction.py:261-278: Dense(h_i, relu) per hidden width,
// a linear Dense(d), then relu(x + h)) stacked n_units times
// (model/deepCrossing.py:15-32), optionally closed by the model's
// Dense(1, sigmoid) head.
//
// Layout and schedule (gfx950), on the fused MLP tower's machinery
// (mlp_tower.hpp: B-fragment packing, weight ring, tile x k-slice work split
// with its fixed-order reduction):
//   * A workgroup owns 16 samples and 16 waves.  The 16 x d input tile is
//     staged in LDS once — from x, or straight from the ids as [dense | rows]
//     (rs_deepcrossing_fwd: the concat is never written) — and every layer of
//     every unit reads its input tile from LDS and writes its result back to
//     LDS (two ping-pong buffers): no activation touches HBM.
//   * The skip operand.  A unit's input must outlive its n_hidden + 1 layers
//     while both buffers are overwritten.  It is held in REGISTERS, by the
//     thread that will finish that element: the last layer of a unit is d wide,
//     so wave w finishes output tiles w, w + 16, ... (<= 4 of them at d <=
//     1024: 16 floats per thread), or, when the layer is narrower than 4
//     tiles and its k-slices meet in LDS, thread e finishes element e of the
//     reduction (1 float).  Each thread reads exactly those elements of the
//     unit's input tile after the barrier that opens the unit's first layer.
//     A third LDS tile would not fit beside two 1024-wide ones (3 x 66 KB);
//     the registers cost nothing at the widths that matter and leave the LDS
//     budget, and so the occupancy, of the plain tower.
//   * The skip-add epilogue relu(x_u + (acc + bias)) runs where the last
//     layer's tile is finished; the padded columns (d..roundup(d,16)) come out
//     as relu(0 + (0 + 0)) = 0 — packed weights, bias and skip are all zero
//     there — so every column a later layer reads has been written.
//   * Biases are read from the packed image (L2) by the finishing lane, the
//     load in flight over the contraction: 16 units' biases need no LDS.
//   * Every sum has one fixed order; a row's result does not depend on the
//     batch or on the row's place in its tile.
#include "mlp_tower.hpp"

namespace rs {

constexpr int RES_MAXH = 4;             // hidden layers per unit
constexpr int RES_MAXL = RES_MAXH + 1;  // ... plus the linear Dense(d)
constexpr int RES_MAXU = 16;            // units per launch
constexpr int RES_NW = MLP_NW;
constexpr int RES_SKIP = MLP_MAXD / 16 / RES_NW;  // output tiles of a d-wide layer per wave

// prepared = [unit_0 .. unit_{U-1} | head_w (dp) | head_b (16)], the head part
// only when head == 1; unit = [W_0 .. W_{nl-1} (packed) | bias_0 .. bias_{nl-1}
// (Np_l each)].  Every block is a multiple of 16 floats.
struct ResGeom {
  int nl, n_units, d, dp;
  int K[RES_MAXL], N[RES_MAXL], Kp[RES_MAXL], Np[RES_MAXL];
  int64_t off[RES_MAXL];   // floats from the unit's base: packed W of layer l
  int64_t boff[RES_MAXL];  // ... bias of layer l
  int64_t unit, head_off, total;
  int rs;      // LDS row stride (floats) of the activation buffers
  size_t lds;  // dynamic LDS bytes
};

static bool res_geom(int d, int n_hidden, const int* hidden, int n_units, int head, ResGeom& g) {
  if (n_hidden < 1 || n_hidden > RES_MAXH || n_units < 1 || n_units > RES_MAXU || !hidden) return false;
  if (d < 1 || d > MLP_MAXD || (head != 0 && head != 1)) return false;
  g.nl = n_hidden + 1;
  g.n_units = n_units;
  g.d = d;
  g.dp = rup(d, 16);
  int maxw = g.dp;
  int64_t off = 0;
  for (int l = 0; l < g.nl; ++l) {
    const int kin = l == 0 ? d : hidden[l - 1], nout = l == n_hidden ? d : hidden[l];
    if (nout < 1 || nout > MLP_MAXD) return false;
    g.K[l] = kin;
    g.N[l] = nout;
    g.Kp[l] = rup(kin, 16);
    g.Np[l] = rup(nout, 16);
    g.off[l] = off;
    off += (int64_t)g.Kp[l] * g.Np[l];
    maxw = std::max(maxw, g.Np[l]);
  }
  for (int l = 0; l < g.nl; ++l) {
    g.boff[l] = off;
    off += g.Np[l];
  }
  g.unit = off;
  g.head_off = off * n_units;
  g.total = g.head_off + (head ? g.dp + 16 : 0);
  g.rs = rup(maxw, 64) + 8;  // 8 (mod 64) dwords: conflict-free ds_read_b128 (mlp_geom)
  g.lds = (size_t)(32 * g.rs + RES_NW * 256) * sizeof(float);
  return g.lds <= 160 * 1024;
}

struct ResPrepArgs {
  const float* W[RES_MAXL];
  const float* bias[RES_MAXL];
  ResGeom g;
  float* out;  // the unit's base
  int trans;   // W[l] is stored [N, K]: pack its transpose (the backward image)
};

__global__ void res_prepare_unit(ResPrepArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.g.unit) return;
  float v = 0.f;
  if (i < a.g.boff[0]) {
    int l = 0;
    while (l + 1 < a.g.nl && i >= a.g.off[l + 1]) ++l;
    const int64_t r = i - a.g.off[l];
    const int K = a.g.K[l], N = a.g.N[l], G = a.g.Kp[l] / 16;
    // lane `lane` of k-group gg, output tile t holds W[16 gg + 4 (lane >> 4) + j][16 t + (lane & 15)]
    const int j = (int)(r & 3), lane = (int)((r >> 2) & 63);
    const int64_t blk = r >> 8;
    const int gg = (int)(blk % G), t = (int)(blk / G);
    const int k = 16 * gg + 4 * (lane >> 4) + j, n = 16 * t + (lane & 15);
    if (k < K && n < N) v = a.trans ? a.W[l][(int64_t)n * K + k] : a.W[l][(int64_t)k * N + n];
  } else {
    int l = 0;
    while (l + 1 < a.g.nl && i >= a.g.boff[l + 1]) ++l;
    const int n = (int)(i - a.g.boff[l]);
    v = (n < a.g.N[l] && a.bias[l]) ? a.bias[l][n] : 0.f;
  }
  a.out[i] = v;
}

__global__ void res_prepare_head(const float* w, const float* b, int d, int dp, float* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= dp + 16) return;
  out[i] = i < d ? (w ? w[i] : 0.f) : (i == dp && b ? b[0] : 0.f);
}

struct ResArgs {
  // the input tile: x [M, d] (KIND 3), or [dense | rows] from the ids
  const float* x;
  int64_t xs;
  const void* ids;
  int64_t id_stride;
  const float* dense;
  int64_t dense_stride;
  int nd;
  const float* table;
  const int64_t* offs;
  const int64_t* vocab;
  int F, k;
  int* err;
  const float* prep;
  int d, dp, nl, n_units, rs, unroll;
  int Kp[RES_MAXL], Np[RES_MAXL];
  int64_t off[RES_MAXL], boff[RES_MAXL], unit, head_off;
  float* xl;  // the last unit's output [M, d], rows xls apart (null: not written)
  int64_t xls;
  float* yh;  // sigmoid(x_L . head_w + head_b) [M], yhs apart (null: no head)
  int64_t yhs;
  int64_t M;
  // the saved-activation forward (SAVE): every layer's true width, the floats
  // one sample takes per unit in `saved`, and the head's logit
  int N[RES_MAXL];
  int64_t sw;
  float* saved;
  float* logit;
};

// this wave's first item of layer l of unit u: its ring, requested early
template <int NW, class Args>
__device__ __forceinline__ void res_first_fill(const Args& a, int u, int l, floatx4 (&ring)[MLP_R]) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int T = a.Np[l] >> 4, G = a.Kp[l] >> 4;
  const int S = mlp_slices(T, G, NW);
  if (w < T * S) {
    const MlpItem it = mlp_item(w, T, G, S);
    mlp_ring_fill(ring,
                  reinterpret_cast<const floatx4*>(a.prep + u * a.unit + a.off[l]) + lane + (int64_t)it.t * G * 64,
                  it.g0, it.g1);
  }
}

__device__ __forceinline__ floatx4 res_pick(const floatx4 (&s)[RES_SKIP], int i) {
  static_assert(RES_SKIP == 4, "four skip tiles per wave");
  return i == 0 ? s[0] : (i == 1 ? s[1] : (i == 2 ? s[2] : s[3]));
}

// SAVE: the training forward — the finishing thread also stores every layer's
// post-activation output (and the staging thread the input tile) to a.saved =
// x_0 [M, d] | unit-major, layer-major a_{u,l} [M, N_l], and the head its logit
template <int NW, int KIND, bool SAVE = false>
__global__ __launch_bounds__(NW * 64) void res_tower(ResArgs a) {
  extern __shared__ float smem[];
  const int RS = a.rs;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t m0 = (int64_t)blockIdx.x * 16;

  // the first layer's weights first (independent of everything), then the
  // input tile, one row per wave; rows past M re-read row M-1 and are never
  // stored; columns d .. dp-1 are zeros
  floatx4 ring[MLP_R];
  res_first_fill<NW>(a, 0, 0, ring);
  for (int r = w; r < 16; r += NW) {
    const int64_t m = m0 + r < a.M ? m0 + r : a.M - 1;
    if constexpr (KIND == 3) {
      const float* xr = a.x + m * a.xs;
      for (int c = lane; c < a.dp; c += 64) {
        const float v = c < a.d ? xr[c] : 0.f;
        smem[r * RS + c] = v;
        if constexpr (SAVE) {
          if (m0 + r < a.M && c < a.d) a.saved[m * a.d + c] = v;
        }
      }
    } else {
      typedef Ids<KIND> I;
      bool bad = false;
      for (int c = lane; c < a.dp; c += 64) {
        float v = 0.f;
        if (c < a.nd) {
          v = a.dense[m * a.dense_stride + c];
        } else if (c < a.d) {
          const int f = (c - a.nd) / a.k, j = (c - a.nd) - f * a.k;
          int64_t id;
          const bool ok = I::decode(I::load(a.ids, m * a.id_stride + f), a.vocab[f], id);
          v = ok ? a.table[(a.offs[f] + id) * a.k + j] : 0.f;
          bad |= !ok;
        }
        smem[r * RS + c] = v;
        if constexpr (SAVE) {
          if (m0 + r < a.M && c < a.d) a.saved[m * a.d + c] = v;
        }
      }
      if (__any(bad) && lane == 0) flag_error(a.err);
    }
  }

  float* in = smem;
  float* out = smem + 16 * RS;
  float* red = smem + 32 * RS;
  const int LL = a.nl - 1;
  // the work split of a unit's last (d-wide) layer decides who holds the skip
  const int TL = a.Np[LL] >> 4;
  const int SL = mlp_slices(TL, a.Kp[LL] >> 4, NW);
  for (int u = 0; u < a.n_units; ++u) {
    const float* up = a.prep + u * a.unit;
    const bool final_unit = u == a.n_units - 1;
    floatx4 skip[RES_SKIP];
#pragma unroll
    for (int i = 0; i < RES_SKIP; ++i) skip[i] = floatx4{0.f, 0.f, 0.f, 0.f};
    int64_t spre = a.d + u * a.sw;  // SAVE: floats per sample before a_{u,l}
    for (int l = 0; l < a.nl; ++l) {
      const int T = a.Np[l] >> 4, G = a.Kp[l] >> 4;
      const int S = mlp_slices(T, G, NW);
      __syncthreads();  // the layer's input complete
      if (l == 0) {
        // the unit's input, by the thread that will add it back (`in` is not
        // written before the next layer's barrier)
        if (SL == 1) {
#pragma unroll
          for (int i = 0; i < RES_SKIP; ++i) {
            const int t = w + NW * i;
            if (t < TL) {
#pragma unroll
              for (int r = 0; r < 4; ++r) skip[i][r] = in[(4 * (lane >> 4) + r) * RS + 16 * t + (lane & 15)];
            }
          }
        } else if ((int)threadIdx.x < TL * 256) {
          const int e = threadIdx.x, t = e >> 8, ln = (e & 255) >> 2, r = e & 3;
          skip[0][0] = in[(4 * (ln >> 4) + r) * RS + 16 * t + (ln & 15)];
        }
      }
      const floatx4* W = reinterpret_cast<const floatx4*>(up + a.off[l]) + lane;
      const float* bias = up + a.boff[l];
      const bool last = l == LL;
      // one finished element: hidden layers relu(v + b); the unit's last layer
      // relu(x_u + (v + b)), also to x_L when this is the last unit
      const int Nl = SAVE ? a.N[l] : 0;
      float* sv = SAVE ? a.saved + a.M * spre : nullptr;  // a_{u,l} [M, Nl]
      spre += Nl;
      auto finish = [&](int row, int col, float v, float bc, float sk) {
        if (!last) {
          const float y = fmaxf(v + bc, 0.f);
          out[row * RS + col] = y;
          if constexpr (SAVE) {
            const int64_t m = m0 + row;
            if (m < a.M && col < Nl) sv[m * Nl + col] = y;
          }
        } else {
          const float y = fmaxf(sk + (v + bc), 0.f);
          out[row * RS + col] = y;
          const int64_t m = m0 + row;
          if (final_unit && a.xl && m < a.M && col < a.d) a.xl[m * a.xls + col] = y;
          if constexpr (SAVE) {
            if (m < a.M && col < Nl) sv[m * Nl + col] = y;
          }
        }
      };

      const float* ap = in + (lane & 15) * RS + 4 * (lane >> 4);
      int i = 0;
      for (int item = w; item < T * S; item += NW, ++i) {
        const MlpItem it = mlp_item(item, T, G, S);
        const floatx4* bp = W + (int64_t)it.t * G * 64;
        if (item != w) mlp_ring_fill(ring, bp, it.g0, it.g1);
        const int col = 16 * it.t + (lane & 15);
        const float bc = bias[col];  // in flight over the contraction
        floatx4 acc = {0.f, 0.f, 0.f, 0.f};
        mlp_mac(ring, ap, bp, it.g0, it.g1, acc, a.unroll);
        if (S == 1) {
          const floatx4 sk = res_pick(skip, i);
#pragma unroll
          for (int r = 0; r < 4; ++r) finish(4 * (lane >> 4) + r, col, acc[r], bc, sk[r]);
        } else {
          *reinterpret_cast<floatx4*>(red + item * 256 + lane * 4) = acc;
        }
      }
      // the next layer's first weights (the next unit's, after the last
      // layer) do not depend on this layer: request them now
      if (l + 1 < a.nl) res_first_fill<NW>(a, u, l + 1, ring);
      else if (!final_unit) res_first_fill<NW>(a, u + 1, 0, ring);
      if (S > 1) {
        __syncthreads();  // the partial tiles in red
        for (int e = threadIdx.x; e < T * 256; e += NW * 64) {
          const int t = e >> 8, q = e & 255, ln = q >> 2, r = q & 3;
          float v = 0.f;
          for (int p = 0; p < S; ++p) v += red[(p * T + t) * 256 + q];
          const int col = 16 * t + (ln & 15);
          finish(4 * (ln >> 4) + r, col, v, bias[col], skip[0][0]);
        }
      }
      float* tmp = in;
      in = out;
      out = tmp;
    }
  }
  if (a.yh) {
    // the head: one sample row per wave, columns in lane order then a fixed
    // butterfly (the padded columns of x_L and of head_w are zeros)
    __syncthreads();
    const float* hw = a.prep + a.head_off;
    for (int r = w; r < 16; r += NW) {
      float z = 0.f;
      for (int c = lane; c < a.dp; c += 64) z = fmaf(in[r * RS + c], hw[c], z);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) z += __shfl_xor(z, o, 64);
      const int64_t m = m0 + r;
      if (lane == 0 && m < a.M) {
        a.yh[m * a.yhs] = sigmoidf_(z + hw[a.dp]);
        if constexpr (SAVE) a.logit[m] = z + hw[a.dp];
      }
    }
  }
}

static void res_fill_args(const ResGeom& g, const float* prepared, ResArgs& a) {
  for (int l = 0; l < g.nl; ++l) {
    a.Kp[l] = g.Kp[l];
    a.Np[l] = g.Np[l];
    a.off[l] = g.off[l];
    a.boff[l] = g.boff[l];
  }
  a.prep = prepared;
  a.d = g.d;
  a.dp = g.dp;
  a.nl = g.nl;
  a.n_units = g.n_units;
  a.rs = g.rs;
  a.unit = g.unit;
  a.head_off = g.head_off;
  a.unroll = opt(RS_OPT_MLP_UNROLL);
}

template <int KIND, bool SAVE = false>
static int res_launch(const ResArgs& a, const ResGeom& g, rs_stream_t stream, const char* what) {
  const int64_t grid = (a.M + 15) / 16;
  RS_REQUIRE(grid < (1ll << 31), "%s: batch too large", what);
  launch_lds<res_tower<RES_NW, KIND, SAVE>>((unsigned)grid, RES_NW * 64, g.lds, as_stream(stream), a);
  return launch_status(what);
}

// ---- Training.  The floats one sample takes per unit in `saved` / `deltas`
// (sum of the hidden widths + d) and the offset of layer l inside them.
struct ResSaved {
  int N[RES_MAXL];
  int64_t pre[RES_MAXL], sw;
};
static ResSaved res_saved(int d, int n_hidden, const int* hidden) {
  ResSaved s{};
  for (int l = 0; l <= n_hidden; ++l) {
    s.N[l] = l == n_hidden ? d : hidden[l];
    s.pre[l] = s.sw;
    s.sw += s.N[l];
  }
  return s;
}
// the geometry of a unit's backward chain: the forward's with `hidden` reversed
static bool res_geom_bwd(int d, int n_hidden, const int* hidden, int n_units, ResGeom& g) {
  if (n_hidden < 1 || n_hidden > RES_MAXH || !hidden) return false;
  int rev[RES_MAXH];
  for (int l = 0; l < n_hidden; ++l) rev[l] = hidden[n_hidden - 1 - l];
  return res_geom(d, n_hidden, rev, n_units, 1, g);
}

// The backward data path of the stack, the forward's launch shape run in
// reverse: image unit i is forward unit u = U-1-i, its chain layer l is
// W_{n_hidden - l}^T (rs_res_tower_prepare_bwd), so the widths are the
// forward's reversed and the last chain layer is d wide again.
//   * Staging: e_u = dy_u [x_{u+1} > 0] for the top unit (dy, or g[b] head_w
//     in the head form), stored as delta_{u,n_hidden}.  It is the first chain
//     layer's input tile AND the skip operand, held in registers exactly as
//     the forward holds x_u.
//   * A hidden step finishes delta_{u,j} = (delta_{u,j+1} W_{j+1}^T) [a_{u,j}
//     > 0]: the mask value comes from `saved`, loaded by the finishing lane
//     over the contraction (where the forward loads the bias).
//   * The d-wide step finishes dy_{u-1} = e_u + delta_{u,0} W_0^T, masked
//     with [x_u > 0] into delta_{u-1,n_hidden} (the next unit's e, left in
//     LDS), or unmasked into dx0 for u = 0.
// Padded columns come out as exact zeros (zero packed weights, zero mask),
// rows past M are computed from row M-1's staging and never stored.
struct ResBwdArgs {
  const float* saved;  // x_0 [M, d] | a_{u,l} [M, N_l]
  const float* dy;     // dL/dx_U [M, d], rows dys apart, or null:
  int64_t dys;
  const float* g;      // ... dL/dx_U = g[m] * head_w (the image's head slot)
  float* deltas;       // delta_{u,l} [M, N_l], the layout of saved without x_0
  float* dx0;          // [M, d], rows dx0s apart
  int64_t dx0s;
  const float* prep;
  int d, dp, nl, n_units, rs, unroll;
  int Kp[RES_MAXL], Np[RES_MAXL];  // of the chain (reversed widths)
  int64_t off[RES_MAXL], unit, head_off;
  int fN[RES_MAXL];       // forward layer widths
  int64_t fpre[RES_MAXL], sw;
  int64_t M;
};

template <int NW>
__global__ __launch_bounds__(NW * 64) void res_tower_bwd(ResBwdArgs a) {
  extern __shared__ float smem[];
  const int RS = a.rs;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t m0 = (int64_t)blockIdx.x * 16;
  const int nh = a.nl - 1, U = a.n_units;
  const float* sv = a.saved + a.M * a.d;  // a_{u,l} at sv + M (u sw + fpre[l]), as delta_{u,l} in deltas

  floatx4 ring[MLP_R];
  res_first_fill<NW>(a, 0, 0, ring);
  {
    const int64_t top = a.M * ((U - 1) * a.sw + a.fpre[nh]);
    const float* hw = a.prep + a.head_off;
    for (int r = w; r < 16; r += NW) {
      const bool live = m0 + r < a.M;
      const int64_t m = live ? m0 + r : a.M - 1;
      const float gm = a.g ? a.g[m] : 0.f;
      for (int c = lane; c < a.dp; c += 64) {
        float v = 0.f;
        if (c < a.d) {
          const float dyv = a.g ? gm * hw[c] : a.dy[m * a.dys + c];
          v = sv[top + m * a.d + c] > 0.f ? dyv : 0.f;
          if (live) a.deltas[top + m * a.d + c] = v;
        }
        smem[r * RS + c] = v;
      }
    }
  }

  float* in = smem;
  float* out = smem + 16 * RS;
  float* red = smem + 32 * RS;
  const int LL = a.nl - 1;
  const int TL = a.Np[LL] >> 4;
  const int SL = mlp_slices(TL, a.Kp[LL] >> 4, NW);
  for (int i = 0; i < U; ++i) {
    const int u = U - 1 - i;
    const float* up = a.prep + i * a.unit;
    floatx4 skip[RES_SKIP];
#pragma unroll
    for (int q = 0; q < RES_SKIP; ++q) skip[q] = floatx4{0.f, 0.f, 0.f, 0.f};
    for (int l = 0; l < a.nl; ++l) {
      const int T = a.Np[l] >> 4, G = a.Kp[l] >> 4;
      const int S = mlp_slices(T, G, NW);
      __syncthreads();  // the layer's input complete
      if (l == 0) {
        // e_u, by the thread that will add it back
        if (SL == 1) {
#pragma unroll
          for (int q = 0; q < RES_SKIP; ++q) {
            const int t = w + NW * q;
            if (t < TL) {
#pragma unroll
              for (int r = 0; r < 4; ++r) skip[q][r] = in[(4 * (lane >> 4) + r) * RS + 16 * t + (lane & 15)];
            }
          }
        } else if ((int)threadIdx.x < TL * 256) {
          const int e = threadIdx.x, t = e >> 8, ln = (e & 255) >> 2, r = e & 3;
          skip[0][0] = in[(4 * (ln >> 4) + r) * RS + 16 * t + (ln & 15)];
        }
      }
      const floatx4* W = reinterpret_cast<const floatx4*>(up + a.off[l]) + lane;
      const bool last = l == LL;
      // what this step finishes: delta_{u,nh-1-l}, or (last) delta_{u-1,nh} / dx0
      const bool masked = !(last && u == 0);
      const int No = last ? a.d : a.fN[nh - 1 - l];
      const int64_t ob = !masked ? 0 : a.M * (last ? (u - 1) * a.sw + a.fpre[nh] : u * a.sw + a.fpre[nh - 1 - l]);
      const float* mp = sv + ob;
      float* dst = masked ? a.deltas + ob : a.dx0;
      const int64_t ds = masked ? No : a.dx0s;
      auto mask_at = [&](int row, int col) {
        const int64_t m = m0 + row;
        return (masked && m < a.M && col < No) ? mp[m * No + col] : 0.f;
      };
      auto finish = [&](int row, int col, float v, float mk, float sk) {
        float y = last ? sk + v : v;
        if (masked) y = mk > 0.f ? y : 0.f;
        out[row * RS + col] = y;
        const int64_t m = m0 + row;
        if (m < a.M && col < No) dst[m * ds + col] = y;
      };

      const float* ap = in + (lane & 15) * RS + 4 * (lane >> 4);
      int q = 0;
      for (int item = w; item < T * S; item += NW, ++q) {
        const MlpItem it = mlp_item(item, T, G, S);
        const floatx4* bp = W + (int64_t)it.t * G * 64;
        if (item != w) mlp_ring_fill(ring, bp, it.g0, it.g1);
        const int col = 16 * it.t + (lane & 15);
        float mk[4] = {0.f, 0.f, 0.f, 0.f};
        if (S == 1) {  // in flight over the contraction
#pragma unroll
          for (int r = 0; r < 4; ++r) mk[r] = mask_at(4 * (lane >> 4) + r, col);
        }
        floatx4 acc = {0.f, 0.f, 0.f, 0.f};
        mlp_mac(ring, ap, bp, it.g0, it.g1, acc, a.unroll);
        if (S == 1) {
          const floatx4 sk = res_pick(skip, q);
#pragma unroll
          for (int r = 0; r < 4; ++r) finish(4 * (lane >> 4) + r, col, acc[r], mk[r], sk[r]);
        } else {
          *reinterpret_cast<floatx4*>(red + item * 256 + lane * 4) = acc;
        }
      }
      if (l + 1 < a.nl) res_first_fill<NW>(a, i, l + 1, ring);
      else if (i + 1 < U) res_first_fill<NW>(a, i + 1, 0, ring);
      if (S > 1) {
        __syncthreads();  // the partial tiles in red
        for (int e = threadIdx.x; e < T * 256; e += NW * 64) {
          const int t = e >> 8, q2 = e & 255, ln = q2 >> 2, r = q2 & 3;
          const int row = 4 * (ln >> 4) + r, col = 16 * t + (ln & 15);
          const float mk = mask_at(row, col);
          float v = 0.f;
          for (int p = 0; p < S; ++p) v += red[(p * T + t) * 256 + q2];
          finish(row, col, v, mk, skip[0][0]);
        }
      }
      float* tmp = in;
      in = out;
      out = tmp;
    }
  }
}

}  // namespace rs

using namespace rs;

#define RES_SHAPE_MSG "need 1..%d hidden widths, 1..%d units, widths 1..%d"

extern "C" int rs_res_tower_ok(int d, int n_hidden, const int* hidden, int n_units) {
  ResGeom g;
  return res_geom(d, n_hidden, hidden, n_units, 0, g) ? 1 : 0;
}

extern "C" int64_t rs_res_tower_prepared_size(int d, int n_hidden, const int* hidden, int n_units, int head) {
  ResGeom g;
  if (!res_geom(d, n_hidden, hidden, n_units, head, g)) {
    set_error("rs_res_tower_prepared_size: " RES_SHAPE_MSG " (head 0 or 1)", RES_MAXH, RES_MAXU, MLP_MAXD);
    return -1;
  }
  return g.total;
}

extern "C" int rs_res_tower_prepare(int d, int n_hidden, const int* hidden, int n_units, const float* const* W,
                                    const float* const* bias, const float* head_w, const float* head_b,
                                    float* prepared, rs_stream_t stream) {
  ResGeom g;
  const int head = head_w ? 1 : 0;
  RS_REQUIRE(res_geom(d, n_hidden, hidden, n_units, head, g), "rs_res_tower_prepare: " RES_SHAPE_MSG, RES_MAXH,
             RES_MAXU, MLP_MAXD);
  RS_REQUIRE(W && prepared, "rs_res_tower_prepare: null pointer");
  RS_REQUIRE(head_w || !head_b, "rs_res_tower_prepare: head_b without head_w");
  for (int i = 0; i < n_units * g.nl; ++i)
    RS_REQUIRE(W[i], "rs_res_tower_prepare: unit %d layer %d has no kernel", i / g.nl, i % g.nl);
  for (int u = 0; u < n_units; ++u) {
    ResPrepArgs a{};
    for (int l = 0; l < g.nl; ++l) {
      a.W[l] = W[u * g.nl + l];
      a.bias[l] = bias ? bias[u * g.nl + l] : nullptr;
    }
    a.g = g;
    a.out = prepared + u * g.unit;
    res_prepare_unit<<<(unsigned)((g.unit + 255) / 256), 256, 0, as_stream(stream)>>>(a);
  }
  if (head)
    res_prepare_head<<<(g.dp + 16 + 255) / 256, 256, 0, as_stream(stream)>>>(head_w, head_b, g.d, g.dp,
                                                                           prepared + g.head_off);
  return launch_status("rs_res_tower_prepare");
}

static void res_fill_saved(int d, int n_hidden, const int* hidden, float* saved, float* logit, ResArgs& a) {
  const ResSaved s = res_saved(d, n_hidden, hidden);
  for (int l = 0; l <= n_hidden; ++l) a.N[l] = s.N[l];
  a.sw = s.sw;
  a.saved = saved;
  a.logit = logit;
}

// rs_res_tower_fwd / rs_res_tower_train_fwd: the checks of the given rows x
// (outs: every output pointer the entry needs is there) and their ResArgs.
static int res_x_source(const char* what, const ResGeom& g, const float* prepared, const float* x, int64_t x_stride,
                        bool outs, int64_t batch, ResArgs& a) {
  RS_REQUIRE(x && prepared && outs, "%s: null pointer", what);
  RS_REQUIRE(batch >= 0 && x_stride >= g.d, "%s: bad batch/stride (x_stride < d)", what);
  res_fill_args(g, prepared, a);
  a.x = x;
  a.xs = x_stride;
  a.M = batch;
  return RS_OK;
}

extern "C" int rs_res_tower_fwd(const float* x, int64_t x_stride, int d, int n_hidden, const int* hidden,
                                int n_units, const float* prepared, int head, float* y, int64_t y_stride,
                                int64_t batch, rs_stream_t stream) {
  if (batch == 0) return RS_OK;  // empty batch: nothing to launch (null data pointers allowed)
  ResGeom g;
  RS_REQUIRE(res_geom(d, n_hidden, hidden, n_units, head, g), "rs_res_tower_fwd: " RES_SHAPE_MSG " (head 0 or 1)",
             RES_MAXH, RES_MAXU, MLP_MAXD);
  ResArgs a{};
  if (const int rc = res_x_source("rs_res_tower_fwd", g, prepared, x, x_stride, y != nullptr, batch, a)) return rc;
  RS_REQUIRE(y_stride >= (head ? 1 : d), "rs_res_tower_fwd: y_stride too small");
  if (head) {
    a.yh = y;
    a.yhs = y_stride;
  } else {
    a.xl = y;
    a.xls = y_stride;
  }
  return res_launch<3>(a, g, stream, "rs_res_tower_fwd");
}

// rs_deepcrossing_fwd (saved = logit = null: inference, x_last optional) and
// rs_deepcrossing_train_fwd (both given, no x_last): the checks, the id source
// of the ResArgs and the launch.
static int deepcrossing_run(const char* what, bool train, const void* ids, int id_kind, int64_t id_stride,
                            const float* dense, int64_t dense_stride, int nd, const float* table,
                            const int64_t* field_offsets, const int64_t* field_vocab, int n_fields, int k,
                            int n_hidden, const int* hidden, int n_units, const float* prepared, float* saved,
                            float* out, float* logit, float* x_last, int64_t x_last_stride, int64_t batch,
                            int* err_flag, rs_stream_t stream) {
  RS_REQUIRE(batch >= 0 && nd >= 0 && n_fields >= 1 && k >= 1 && n_fields <= MLP_MAXD && k <= MLP_MAXD,
             "%s: bad shape", what);
  const int d = nd + n_fields * k;
  ResGeom g;
  RS_REQUIRE(res_geom(d, n_hidden, hidden, n_units, 1, g), "%s: " RES_SHAPE_MSG " (input width nd + n_fields * k)",
             what, RES_MAXH, RES_MAXU, MLP_MAXD);
  RS_REQUIRE(ids && table && field_offsets && field_vocab && prepared && out && (!train || (saved && logit)) &&
                 (nd == 0 || dense),
             "%s: null pointer", what);
  RS_REQUIRE(id_kind >= RS_ID_I32 && id_kind <= RS_ID_F32, "%s: bad id_kind", what);
  RS_REQUIRE(id_stride >= n_fields && (nd == 0 || dense_stride >= nd),
             "%s: id_stride / dense_stride smaller than the width", what);
  RS_REQUIRE(!x_last || x_last_stride >= d, "%s: x_last_stride too small", what);
  RS_REQUIRE((uintptr_t)table % 16 == 0, "%s: table must be 16-B aligned", what);
  ResArgs a{};
  res_fill_args(g, prepared, a);
  if (train) res_fill_saved(d, n_hidden, hidden, saved, logit, a);
  a.ids = ids;
  a.id_stride = id_stride;
  a.dense = dense;
  a.dense_stride = dense_stride;
  a.nd = nd;
  a.table = table;
  a.offs = field_offsets;
  a.vocab = field_vocab;
  a.F = n_fields;
  a.k = k;
  a.err = err_flag;
  a.xl = x_last;
  a.xls = x_last_stride;
  a.yh = out;
  a.yhs = 1;
  a.M = batch;
  int st = RS_OK;
  with_id_kind(id_kind, [&](auto K) {
    constexpr int KIND = decltype(K)::value;
    st = train ? res_launch<KIND, true>(a, g, stream, what) : res_launch<KIND>(a, g, stream, what);
  });
  return st;
}

extern "C" int rs_deepcrossing_fwd(const void* ids, int id_kind, int64_t id_stride, const float* dense,
                                   int64_t dense_stride, int nd, const float* table, const int64_t* field_offsets,
                                   const int64_t* field_vocab, int n_fields, int k, int n_hidden, const int* hidden,
                                   int n_units, const float* prepared, float* out, float* x_last,
                                   int64_t x_last_stride, int64_t batch, int* err_flag, rs_stream_t stream) {
  if (batch == 0) return RS_OK;  // empty batch: nothing to launch (null data pointers allowed)
  return deepcrossing_run("rs_deepcrossing_fwd", false, ids, id_kind, id_stride, dense, dense_stride, nd, table,
                          field_offsets, field_vocab, n_fields, k, n_hidden, hidden, n_units, prepared, nullptr, out,
                          nullptr, x_last, x_last_stride, batch, err_flag, stream);
}

// ------------------------------------------------------------------ training
extern "C" int64_t rs_res_tower_saved_size(int d, int n_hidden, const int* hidden, int n_units, int64_t batch) {
  ResGeom g;
  if (!res_geom(d, n_hidden, hidden, n_units, 1, g) || batch < 0) {
    set_error("rs_res_tower_saved_size: " RES_SHAPE_MSG ", batch >= 0", RES_MAXH, RES_MAXU, MLP_MAXD);
    return -1;
  }
  return batch * (d + n_units * res_saved(d, n_hidden, hidden).sw);
}

extern "C" int rs_res_tower_train_fwd(const float* x, int64_t x_stride, int d, int n_hidden, const int* hidden,
                                      int n_units, const float* prepared, float* saved, float* out, float* logit,
                                      int64_t batch, rs_stream_t stream) {
  if (batch == 0) return RS_OK;  // empty batch: nothing to launch (null data pointers allowed)
  ResGeom g;
  RS_REQUIRE(res_geom(d, n_hidden, hidden, n_units, 1, g), "rs_res_tower_train_fwd: " RES_SHAPE_MSG, RES_MAXH,
             RES_MAXU, MLP_MAXD);
  ResArgs a{};
  if (const int rc =
          res_x_source("rs_res_tower_train_fwd", g, prepared, x, x_stride, saved && out && logit, batch, a))
    return rc;
  res_fill_saved(d, n_hidden, hidden, saved, logit, a);
  a.yh = out;
  a.yhs = 1;
  return res_launch<3, true>(a, g, stream, "rs_res_tower_train_fwd");
}

extern "C" int rs_deepcrossing_train_fwd(const void* ids, int id_kind, int64_t id_stride, const float* dense,
                                         int64_t dense_stride, int nd, const float* table,
                                         const int64_t* field_offsets, const int64_t* field_vocab, int n_fields,
                                         int k, int n_hidden, const int* hidden, int n_units, const float* prepared,
                                         float* saved, float* out, float* logit, int64_t batch, int* err_flag,
                                         rs_stream_t stream) {
  if (batch == 0) return RS_OK;  // empty batch: nothing to launch (null data pointers allowed)
  return deepcrossing_run("rs_deepcrossing_train_fwd", true, ids, id_kind, id_stride, dense, dense_stride, nd, table,
                          field_offsets, field_vocab, n_fields, k, n_hidden, hidden, n_units, prepared, saved, out,
                          logit, nullptr, 0, batch, err_flag, stream);
}

extern "C" int64_t rs_res_tower_bwd_prepared_size(int d, int n_hidden, const int* hidden, int n_units) {
  ResGeom g;
  if (!res_geom_bwd(d, n_hidden, hidden, n_units, g)) {
    set_error("rs_res_tower_bwd_prepared_size: " RES_SHAPE_MSG, RES_MAXH, RES_MAXU, MLP_MAXD);
    return -1;
  }
  return g.total;
}

extern "C" int rs_res_tower_prepare_bwd(int d, int n_hidden, const int* hidden, int n_units, const float* const* W,
                                        const float* head_w, float* prepared, rs_stream_t stream) {
  ResGeom g;
  RS_REQUIRE(res_geom_bwd(d, n_hidden, hidden, n_units, g), "rs_res_tower_prepare_bwd: " RES_SHAPE_MSG, RES_MAXH,
             RES_MAXU, MLP_MAXD);
  RS_REQUIRE(W && prepared, "rs_res_tower_prepare_bwd: null pointer");
  for (int i = 0; i < n_units * g.nl; ++i)
    RS_REQUIRE(W[i], "rs_res_tower_prepare_bwd: unit %d layer %d has no kernel", i / g.nl, i % g.nl);
  for (int i = 0; i < n_units; ++i) {
    // image unit i = forward unit n_units-1-i; chain layer l = W_{n_hidden-l}^T; no biases
    ResPrepArgs a{};
    for (int l = 0; l < g.nl; ++l) a.W[l] = W[(n_units - 1 - i) * g.nl + (n_hidden - l)];
    a.g = g;
    a.out = prepared + i * g.unit;
    a.trans = 1;
    res_prepare_unit<<<(unsigned)((g.unit + 255) / 256), 256, 0, as_stream(stream)>>>(a);
  }
  // the head slot is always there (head_w NULL: zeros, an image for the dy form only)
  res_prepare_head<<<(g.dp + 16 + 255) / 256, 256, 0, as_stream(stream)>>>(head_w, nullptr, g.d, g.dp,
                                                                         prepared + g.head_off);
  return launch_status("rs_res_tower_prepare_bwd");
}

extern "C" int rs_res_tower_bwd(const float* saved, int d, int n_hidden, const int* hidden, int n_units,
                                const float* prepared_bwd, const float* dy, int64_t dy_stride, const float* g,
                                float* deltas, float* dx0, int64_t dx0_stride, int64_t batch, rs_stream_t stream) {
  if (batch == 0) return RS_OK;  // empty batch: nothing to launch (null data pointers allowed)
  ResGeom gm;
  RS_REQUIRE(res_geom_bwd(d, n_hidden, hidden, n_units, gm), "rs_res_tower_bwd: " RES_SHAPE_MSG, RES_MAXH, RES_MAXU,
             MLP_MAXD);
  RS_REQUIRE(saved && prepared_bwd && deltas && dx0, "rs_res_tower_bwd: null pointer");
  RS_REQUIRE((dy != nullptr) != (g != nullptr), "rs_res_tower_bwd: exactly one of dy and g");
  RS_REQUIRE(batch >= 0 && dx0_stride >= d && (!dy || dy_stride >= d),
             "rs_res_tower_bwd: bad batch/stride (dy_stride or dx0_stride < d)");
  const int64_t grid = (batch + 15) / 16;
  RS_REQUIRE(grid < (1ll << 31), "rs_res_tower_bwd: batch too large");
  ResBwdArgs a{};
  for (int l = 0; l < gm.nl; ++l) {
    a.Kp[l] = gm.Kp[l];
    a.Np[l] = gm.Np[l];
    a.off[l] = gm.off[l];
  }
  const ResSaved s = res_saved(d, n_hidden, hidden);
  for (int l = 0; l <= n_hidden; ++l) {
    a.fN[l] = s.N[l];
    a.fpre[l] = s.pre[l];
  }
  a.sw = s.sw;
  a.saved = saved;
  a.dy = dy;
  a.dys = dy_stride;
  a.g = g;
  a.deltas = deltas;
  a.dx0 = dx0;
  a.dx0s = dx0_stride;
  a.prep = prepared_bwd;
  a.d = gm.d;
  a.dp = gm.dp;
  a.nl = gm.nl;
  a.n_units = gm.n_units;
  a.rs = gm.rs;
  a.unit = gm.unit;
  a.head_off = gm.head_off;
  a.unroll = opt(RS_OPT_MLP_UNROLL);
  a.M = batch;
  launch_lds<res_tower_bwd<RES_NW>>((unsigned)grid, RES_NW * 64, gm.lds, as_stream(stream), a);
  return launch_status("rs_res_tower_bwd");
}
