// mmoe.hpp — the multi-gate mixture-of-experts machinery shared by the forward
// (mmoe.hip) and the training entries (mmoe_train.hip): the geometry, the
// packed-element map, the block-diagonal layer on a 16-row tile and the
// one-launch forward kernel itself (SAVE = the training forward, which also
// stores what the backward reads).  See mmoe.hip for the design.
#pragma once
#include "mlp_tower.hpp"

namespace rs {

constexpr int MMOE_MAXE = 16;  // experts
constexpr int MMOE_MAXT = 8;   // tasks
constexpr int MMOE_MAXL = 4;   // tower layers (hidden + output)
constexpr int MMOE_NW = MLP_NW;

// prepared = [W1 (dp N1p, packed) | b1 (N1p) | layer_0 .. layer_{L-1}], layer_l
// = [task 0 .. T-1: W (Kp_l Np_l, packed) | task 0 .. T-1: bias (Np_l)].
struct MmoeGeom {
  int d, dp, H, Hs, Hp, E, T, L, N1, N1p;
  int K[MMOE_MAXL], N[MMOE_MAXL], Kp[MMOE_MAXL], Np[MMOE_MAXL];
  int64_t b1off, off[MMOE_MAXL], boff[MMOE_MAXL], total;
  int zg;      // LDS column of the gate logits in z
  int rs;      // LDS row stride (floats)
  size_t lds;  // dynamic LDS bytes
};

static bool mmoe_geom(int d, int hidden, int n_experts, int n_tasks, int n_tower_layers, const int* tower_dims,
                      MmoeGeom& g) {
  if (d < 1 || d > MLP_MAXD || hidden < 1 || hidden > MLP_MAXD) return false;
  if (n_experts < 1 || n_experts > MMOE_MAXE || n_tasks < 1 || n_tasks > MMOE_MAXT) return false;
  if (n_tower_layers < 0 || n_tower_layers > MMOE_MAXL) return false;
  if (n_tower_layers > 0 && (!tower_dims || tower_dims[0] != hidden)) return false;
  g.d = d;
  g.dp = rup(d, 16);
  g.H = hidden;
  g.Hs = hidden | 1;
  g.Hp = rup(hidden, 16);
  g.E = n_experts;
  g.T = n_tasks;
  g.L = n_tower_layers;
  g.N1 = (hidden + n_tasks) * n_experts;
  g.N1p = rup(g.N1, 16);
  if (g.N1p > MLP_MAXD) return false;
  g.zg = g.E * g.Hs;
  int maxw = std::max(std::max(g.dp, g.zg + g.T * g.E), g.T * g.Hp);
  g.b1off = (int64_t)g.dp * g.N1p;
  int64_t off = g.b1off + g.N1p;
  for (int l = 0; l < g.L; ++l) {
    const int kin = tower_dims[l], nout = tower_dims[l + 1];
    if (kin < 1 || kin > MLP_MAXD || nout < 1 || nout > MLP_MAXD) return false;
    g.K[l] = kin;
    g.N[l] = nout;
    g.Kp[l] = rup(kin, 16);
    g.Np[l] = rup(nout, 16);
    g.off[l] = off;
    off += (int64_t)g.T * g.Kp[l] * g.Np[l];
    g.boff[l] = off;
    off += (int64_t)g.T * g.Np[l];
    maxw = std::max(maxw, g.T * std::max(g.Kp[l], g.Np[l]));
  }
  g.total = off;
  g.rs = rup(maxw, 64) + 8;  // 8 (mod 64) dwords: conflict-free ds_read_b128 (mlp_geom)
  g.lds = (size_t)(32 * g.rs + MMOE_NW * 256) * sizeof(float);
  return g.lds <= 160 * 1024;
}

// the (k, n) a packed element r holds: lane `lane` of k-group gg, output tile t
// holds W[16 gg + 4 (lane >> 4) + j][16 t + (lane & 15)]
__device__ __forceinline__ void mmoe_unpack(int64_t r, int G, int& k, int& n) {
  const int j = (int)(r & 3), lane = (int)((r >> 2) & 63);
  const int64_t blk = r >> 8;
  const int gg = (int)(blk % G), t = (int)(blk / G);
  k = 16 * gg + 4 * (lane >> 4) + j;
  n = 16 * t + (lane & 15);
}

struct MmoeArgs {
  const float* x;
  int64_t xs;
  const float* prep;
  int d, dp, H, Hs, Hp, E, T, L, N1, N1p, zg, rs, unroll;
  int Kp[MMOE_MAXL], Np[MMOE_MAXL], act[MMOE_MAXL];
  int64_t b1off, off[MMOE_MAXL], boff[MMOE_MAXL];
  int Nout;     // the towers' output_dim
  float* mix;   // [M, T H], rows mixs apart (null: not written)
  int64_t mixs;
  float* y;     // task t at y + t yts: [M, Nout], rows ys apart
  int64_t yts, ys;
  int64_t M;
  // SAVE only (rs_mmoe_train_fwd), dense row-major blocks of `saved`:
  int N[MMOE_MAXL];
  float* sv_exp;             // relu experts [M, H E], column h E + e
  float* sv_gate;            // gates [M, T E]
  float* sv_a[MMOE_MAXL];    // hidden tower layer l's output [M, T N_l], task t at columns t N_l
};

// this wave's first item of a layer of TT tiles x G k-groups at W: its ring
template <int NW>
__device__ __forceinline__ void mmoe_first_fill(const float* W, int TT, int G, floatx4 (&ring)[MLP_R]) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int S = mlp_slices(TT, G, NW);
  if (w < TT * S) {
    const MlpItem it = mlp_item(w, TT, G, S);
    mlp_ring_fill(ring, reinterpret_cast<const floatx4*>(W) + lane + (int64_t)it.t * G * 64, it.g0, it.g1);
  }
}

// One block-diagonal layer on the 16-row tile: TT output tiles of G k-groups
// each, tile tt contracting the A columns acol(tt) .. + 16 G of `in` (written,
// barrier taken by the caller) with its packed weights at W; fin(row, col, v,
// bias) receives every finished element (BIAS false: the image holds no
// biases, `bias` is not read and fin gets 0).  `next`: the following layer's
// first ring fill, issued before the reduction's barrier.
template <int NW, bool BIAS = true, class ACol, class Fin, class Next>
__device__ __forceinline__ void mmoe_layer(const float* W, const float* bias, int TT, int G, const float* in, int RS,
                                           float* red, floatx4 (&ring)[MLP_R], int unroll, ACol acol, Fin fin,
                                           Next next) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int S = mlp_slices(TT, G, NW);
  const floatx4* Wl = reinterpret_cast<const floatx4*>(W) + lane;
  for (int item = w; item < TT * S; item += NW) {
    const MlpItem it = mlp_item(item, TT, G, S);
    const floatx4* bp = Wl + (int64_t)it.t * G * 64;
    if (item != w) mlp_ring_fill(ring, bp, it.g0, it.g1);
    const int col = 16 * it.t + (lane & 15);
    float bc = 0.f;
    if constexpr (BIAS) bc = bias[col];  // in flight over the contraction
    const float* ap = in + (lane & 15) * RS + 4 * (lane >> 4) + acol(it.t);
    floatx4 acc = {0.f, 0.f, 0.f, 0.f};
    mlp_mac(ring, ap, bp, it.g0, it.g1, acc, unroll);
    if (S == 1) {
#pragma unroll
      for (int r = 0; r < 4; ++r) fin(4 * (lane >> 4) + r, col, acc[r], bc);
    } else {
      *reinterpret_cast<floatx4*>(red + item * 256 + lane * 4) = acc;  // TT < 4: TT S <= NW items
    }
  }
  next();
  if (S > 1) {
    __syncthreads();  // the partial tiles in red
    for (int e = threadIdx.x; e < TT * 256; e += NW * 64) {
      const int t = e >> 8, q = e & 255, ln = q >> 2, r = q & 3;
      float v = 0.f;
      for (int p = 0; p < S; ++p) v += red[(p * TT + t) * 256 + q];
      const int col = 16 * t + (ln & 15);
      float bc = 0.f;
      if constexpr (BIAS) bc = bias[col];
      fin(4 * (ln >> 4) + r, col, v, bc);
    }
  }
}

// SAVE: the same launch also stores the relu experts, the gates, the mixes
// (through a.mix) and every hidden tower layer's output — the same values it
// goes on with, so y does not change.
template <int NW, bool SAVE = false>
__global__ __launch_bounds__(NW * 64) void mmoe_fwd(MmoeArgs a) {
  extern __shared__ float smem[];
  const int RS = a.rs;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t m0 = (int64_t)blockIdx.x * 16;
  float* buf0 = smem;
  float* buf1 = smem + 16 * RS;
  float* red = smem + 32 * RS;

  // stage 1's weights first (independent of everything), then the input tile,
  // one row per wave; columns d .. dp-1 are zeros
  floatx4 ring[MLP_R];
  mmoe_first_fill<NW>(a.prep, a.N1p >> 4, a.dp >> 4, ring);
  for (int r = w; r < 16; r += NW) {
    const int64_t m = m0 + r < a.M ? m0 + r : a.M - 1;
    const float* xr = a.x + m * a.xs;
    for (int c = lane; c < a.dp; c += 64) buf0[r * RS + c] = c < a.d ? xr[c] : 0.f;
  }
  auto fill_tower = [&](int l) {
    if (l < a.L) mmoe_first_fill<NW>(a.prep + a.off[l], a.T * (a.Np[l] >> 4), a.Kp[l] >> 4, ring);
  };

  // ---- stage 1: z = [relu experts, transposed | gate logits] in buf1
  __syncthreads();
  {
    const int HE = a.H * a.E;
    mmoe_layer<NW>(
        a.prep, a.prep + a.b1off, a.N1p >> 4, a.dp >> 4, buf0, RS, red, ring, a.unroll, [](int) { return 0; },
        [&](int row, int col, float v, float bc) {
          if (col < HE) {
            const int h = col / a.E, e = col - h * a.E;
            const float ev = fmaxf(v + bc, 0.f);
            buf1[row * RS + e * a.Hs + h] = ev;
            if constexpr (SAVE) {
              const int64_t m = m0 + row;
              if (m < a.M) a.sv_exp[m * HE + col] = ev;
            }
          } else if (col < a.N1) {
            buf1[row * RS + a.zg + (col - HE)] = v + bc;
          }
        },
        [&] { fill_tower(0); });
  }

  // ---- stage 2: per (row, task) softmax over the experts, the gated mix
  __syncthreads();
  {
    const int TH = a.T * a.Hp, E = a.E;
    for (int i = threadIdx.x; i < 16 * TH; i += NW * 64) {
      const int row = i / TH, j = i - row * TH, t = j / a.Hp, h = j - t * a.Hp;
      float v = 0.f;
      if (h < a.H) {
        const float* zr = buf1 + row * RS;
        const float* gp = zr + a.zg + t * E;  // (one address per row and task: a broadcast)
        float mx = gp[0];
        for (int e = 1; e < E; ++e) mx = fmaxf(mx, gp[e]);
        float p[MMOE_MAXE];
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < MMOE_MAXE; ++e) {
          p[e] = e < E ? expf(gp[e] - mx) : 0.f;
          s += p[e];  // (+ 0 past E: exact)
        }
#pragma unroll
        for (int e = 0; e < MMOE_MAXE; ++e) {
          if (e < E) v = fmaf(p[e] / s, zr[e * a.Hs + h], v);
        }
        const int64_t m = m0 + row;
        if (a.mix && m < a.M) a.mix[m * a.mixs + t * a.H + h] = v;
        if constexpr (SAVE) {
          if (h == 0 && m < a.M) {
#pragma unroll
            for (int e = 0; e < MMOE_MAXE; ++e) {
              if (e < E) a.sv_gate[m * (a.T * E) + t * E + e] = p[e] / s;
            }
          }
        }
      }
      buf0[row * RS + j] = v;  // (columns H .. Hp-1 of a task: zeros)
    }
  }

  // ---- stage 3: the towers, layer l of every task as one layer
  float* in = buf0;
  float* out = buf1;
  for (int l = 0; l < a.L; ++l) {
    const int Tl = a.Np[l] >> 4, Kp = a.Kp[l], Np = a.Np[l];
    const bool last = l == a.L - 1;
    __syncthreads();  // the layer's input complete
    with_act(a.act[l], [&](auto A) {
      mmoe_layer<NW>(
          a.prep + a.off[l], a.prep + a.boff[l], a.T * Tl, Kp >> 4, in, RS, red, ring, a.unroll,
          [&](int tt) { return (tt / Tl) * Kp; },
          [&](int row, int col, float v, float bc) {
            const float yv = mlp_act_c<decltype(A)::value>(v + bc, 0.f);
            if (!last) {
              out[row * RS + col] = yv;
              if constexpr (SAVE) {
                const int t = col / Np, n = col - t * Np;
                const int64_t m = m0 + row;
                if (m < a.M && n < a.N[l]) a.sv_a[l][(m * a.T + t) * a.N[l] + n] = yv;
              }
            } else {
              const int t = col / Np, n = col - t * Np;
              const int64_t m = m0 + row;
              if (m < a.M && n < a.Nout) a.y[t * a.yts + m * a.ys + n] = yv;
            }
          },
          [&] { fill_tower(l + 1); });
    });
    float* tmp = in;
    in = out;
    out = tmp;
  }
}

#define MMOE_SHAPE_MSG                                                                                           \
  "need d, hidden 1..%d, 1..%d experts, 1..%d tasks, (hidden + tasks) * experts <= %d, 0..%d tower layers with " \
  "widths 1..%d and tower_dims[0] == hidden, and a tile that fits the LDS"
#define MMOE_SHAPE_ARGS MLP_MAXD, MMOE_MAXE, MMOE_MAXT, MLP_MAXD, MMOE_MAXL, MLP_MAXD

// The floats one sample takes in `saved` and where its blocks start (in units
// of one sample's floats): [expert H E | gates T E | mix T H | a_0 .. a_{L-2}].
struct MmoeSaved {
  int64_t gate, mix, a[MMOE_MAXL], per;
};
static MmoeSaved mmoe_saved(const MmoeGeom& g) {
  MmoeSaved s{};
  s.gate = (int64_t)g.H * g.E;
  s.mix = s.gate + (int64_t)g.T * g.E;
  int64_t off = s.mix + (int64_t)g.T * g.H;
  for (int l = 0; l + 1 < g.L; ++l) {
    s.a[l] = off;
    off += (int64_t)g.T * g.N[l];
  }
  s.per = off;
  return s;
}

// rs_mmoe_fwd (saved null) / rs_mmoe_train_fwd: validation, arguments, launch.
template <bool SAVE>
static int mmoe_fwd_run(const char* what, const float* x, int64_t x_stride, int d, int hidden, int n_experts,
                        int n_tasks, int n_tower_layers, const int* tower_dims, const int* tower_acts,
                        const float* prepared, float* mix, int64_t mix_stride, float* y, int64_t y_task_stride,
                        int64_t y_stride, float* saved, int64_t batch, rs_stream_t stream) {
  MmoeGeom g;
  RS_REQUIRE(mmoe_geom(d, hidden, n_experts, n_tasks, n_tower_layers, tower_dims, g), "%s: " MMOE_SHAPE_MSG, what,
             MMOE_SHAPE_ARGS);
  RS_REQUIRE(x && prepared, "%s: null pointer (x, prepared)", what);
  RS_REQUIRE(g.L > 0 || mix, "%s: null pointer (n_tower_layers 0 is the layer alone: mix is its output)", what);
  RS_REQUIRE(g.L == 0 || (y && tower_acts), "%s: null pointer (y, tower_acts)", what);
  RS_REQUIRE(batch > 0 && x_stride >= d, "%s: bad batch/stride (x_stride < d)", what);
  RS_REQUIRE(!mix || mix_stride >= (int64_t)g.T * g.H, "%s: mix_stride smaller than n_tasks * hidden", what);
  MmoeArgs a{};
  if (g.L > 0) {
    a.Nout = g.N[g.L - 1];
    RS_REQUIRE(y_stride >= a.Nout && y_task_stride >= a.Nout,
               "%s: y_stride / y_task_stride smaller than the output width", what);
  }
  for (int l = 0; l < g.L; ++l) {
    // (no PReLU: tower_layer's Dense has no alpha, and the image holds none)
    RS_REQUIRE(tower_acts[l] == RS_ACT_NONE || tower_acts[l] == RS_ACT_RELU || tower_acts[l] == RS_ACT_SIGMOID,
               "%s: tower activation %d of layer %d (none, relu or sigmoid)", what, tower_acts[l], l);
    a.Kp[l] = g.Kp[l];
    a.Np[l] = g.Np[l];
    a.N[l] = g.N[l];
    a.act[l] = tower_acts[l];
    a.off[l] = g.off[l];
    a.boff[l] = g.boff[l];
  }
  const int64_t grid = (batch + 15) / 16;
  RS_REQUIRE(grid < (1ll << 31), "%s: batch too large", what);
  a.x = x;
  a.xs = x_stride;
  a.prep = prepared;
  a.d = g.d;
  a.dp = g.dp;
  a.H = g.H;
  a.Hs = g.Hs;
  a.Hp = g.Hp;
  a.E = g.E;
  a.T = g.T;
  a.L = g.L;
  a.N1 = g.N1;
  a.N1p = g.N1p;
  a.zg = g.zg;
  a.rs = g.rs;
  a.unroll = opt(RS_OPT_MLP_UNROLL);
  a.b1off = g.b1off;
  a.mix = mix;
  a.mixs = mix_stride;
  a.y = y;
  a.yts = y_task_stride;
  a.ys = y_stride;
  a.M = batch;
  if constexpr (SAVE) {
    const MmoeSaved s = mmoe_saved(g);
    a.sv_exp = saved;
    a.sv_gate = saved + batch * s.gate;
    a.mix = saved + batch * s.mix;
    a.mixs = (int64_t)g.T * g.H;
    for (int l = 0; l + 1 < g.L; ++l) a.sv_a[l] = saved + batch * s.a[l];
  }
  launch_lds<mmoe_fwd<MMOE_NW, SAVE>>((unsigned)grid, MMOE_NW * 64, g.lds, as_stream(stream), a);
  return launch_status(what);
}

}  // namespace rs
