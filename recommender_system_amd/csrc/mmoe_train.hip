// mmoe_train.hip — training MMOE (MMOE.train_step): the forward that also
// stores what the backward reads (mmoe_fwd<SAVE>, mmoe.hpp), the per-task
// sigmoid cross-entropy head, and the whole backward data path in one launch.
//
// The backward (mmoe_bwd), the forward's launch shape run in reverse — a
// workgroup owns 16 samples and 16 waves, three LDS tiles [16][rs] and the
// partial-tile area:
//   * Staging.  G [16, T Nout] goes to tile A at column t Np_{L-1} + j (the
//     top layer's padded width), the saved relu experts and gates to tile C
//     in the forward's stage-1 column order (expert (h, e) at h E + e, gate
//     (t, e) at H E + t E + e): the order dz1 has, so the expert part below
//     reads, writes and stores consecutive columns from consecutive lanes, and
//     the gate reduction reads E consecutive floats per (row, task).
//   * Towers.  For l = L-1 .. 0 the T tasks' W_{t,l}^T are ONE block-diagonal
//     layer (mmoe_layer<>, no biases: image chain layer l = the tasks' packed
//     [Np_l, Kp_l] transposes one after another): delta_{l-1} = (delta_l
//     W_l^T) [a_{l-1} > 0], the mask read from `saved` by the finishing lane,
//     stored to `deltas` and left in LDS as the next layer's input; l = 0
//     leaves dmix [16, T Hp], which is never stored.
//   * Gates.  dp_t[e] = sum_h dmix_t[h] expert[h, e] (h ascending), one thread
//     per (row, task, e), into the partial-tile area; then dlogit_t[e] =
//     p_t[e] (dp_t[e] - sum_e' p_t[e'] dp_t[e']) (e' ascending).
//   * Experts.  dexp[h, e] = [expert[h, e] > 0] sum_t p_t[e] dmix_t[h] (t
//     ascending), one thread per (row, column).
//   * dz1 = [dexp | dlogit] is stored and left in LDS (padded to N1p with
//     zeros) as the A tile of dx = dz1 W1^T (K = N1p, dp / 16 output tiles),
//     skipped when dx is not asked for.
// Every sum has one fixed order and no atomics; rows past the batch re-read
// the last row and are never stored, so a row's result does not depend on the
// batch or on its place in the tile.
#include "mmoe.hpp"

namespace rs {

// prepared_bwd = [chain layer L-1 .. 0 | W1^T]: chain layer l = task 0 .. T-1:
// W_{t,l}^T (Np_l x Kp_l, packed); W1^T (N1p x dp, packed), rows in the
// forward's stage-1 column order.
struct MmoeTrainGeom {
  MmoeGeom f;
  int rs;
  size_t lds;
  int64_t woff[MMOE_MAXL], w1off, total;
};

static bool mmoe_train_geom(int d, int hidden, int n_experts, int n_tasks, int n_tower_layers, const int* tower_dims,
                            MmoeTrainGeom& g) {
  if (n_tower_layers < 1 || !mmoe_geom(d, hidden, n_experts, n_tasks, n_tower_layers, tower_dims, g.f)) return false;
  const MmoeGeom& f = g.f;
  int maxw = std::max(std::max(f.dp, f.N1p), f.T * f.Hp);
  int64_t off = 0;
  for (int l = f.L - 1; l >= 0; --l) {
    maxw = std::max(maxw, f.T * std::max(f.Kp[l], f.Np[l]));
    g.woff[l] = off;
    off += (int64_t)f.T * f.Kp[l] * f.Np[l];
  }
  g.w1off = off;
  g.total = off + (int64_t)f.N1p * f.dp;
  g.rs = rup(maxw, 64) + 8;  // 8 (mod 64) dwords, as the forward's
  g.lds = (size_t)(48 * g.rs + MMOE_NW * 256) * sizeof(float);
  return g.lds <= 160 * 1024;
}

struct MmoePrepBwdLayerArgs {
  const float* W[MMOE_MAXT];  // task t's kernel [K, N]
  int K, N, Kp, Np, T;
  float* out;
};

// element (k', n') of task t's chain layer = W_t[n'][k']
__global__ void mmoe_prepare_bwd_layer(MmoePrepBwdLayerArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t per = (int64_t)a.Kp * a.Np;
  if (i >= per * a.T) return;
  const int t = (int)(i / per);
  int k, n;
  mmoe_unpack(i - t * per, a.Np / 16, k, n);
  a.out[i] = (k < a.N && n < a.K) ? a.W[t][(int64_t)n * a.N + k] : 0.f;
}

struct MmoePrepBwd1Args {
  const float* ew;             // [d, H E]
  const float* gw[MMOE_MAXT];  // [d, E]
  int d, dp, HE, E, N1, N1p;
  float* out;
};

// element (c, n) of W1^T = stage-1 column c of input n
__global__ void mmoe_prepare_bwd_stage1(MmoePrepBwd1Args a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)a.N1p * a.dp) return;
  int c, n;
  mmoe_unpack(i, a.N1p / 16, c, n);
  float v = 0.f;
  if (n < a.d && c < a.HE) {
    v = a.ew[(int64_t)n * a.HE + c];
  } else if (n < a.d && c < a.N1) {
    const int t = (c - a.HE) / a.E, e = (c - a.HE) - t * a.E;
    v = a.gw[t][(int64_t)n * a.E + e];
  }
  a.out[i] = v;
}

struct MmoeHeadArgs {
  const float* z;  // task t's logits [M, Nout] at z + t zts, rows zs apart
  int64_t zts, zs;
  const float* y;  // labels, the same addressing
  int64_t yts, ys;
  float w[MMOE_MAXT];
  int Nout, T;
  int64_t M;
  float* G;  // [M, T Nout], rows Gs apart
  int64_t Gs;
  float* loss;  // [T, M] or null
};

// one thread per (task, sample): G = w_t (sigmoid(z) - y) / (M Nout), loss =
// mean_j (max(z, 0) - z y + log1p(exp(-|z|))), j ascending
__global__ void mmoe_head_grad(MmoeHeadArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.M * a.T) return;
  const int t = (int)(i / a.M);
  const int64_t m = i - t * a.M;
  const float den = (float)a.M * (float)a.Nout;
  const float* zr = a.z + t * a.zts + m * a.zs;
  const float* yr = a.y + t * a.yts + m * a.ys;
  float* gr = a.G + m * a.Gs + t * a.Nout;
  float acc = 0.f;
  for (int j = 0; j < a.Nout; ++j) {
    const float z = zr[j], y = yr[j];
    const float s = 1.0f / (1.0f + expf(-z));
    gr[j] = a.w[t] * (s - y) / den;
    acc += fmaxf(z, 0.f) - z * y + log1pf(expf(-fabsf(z)));
  }
  if (a.loss) a.loss[i] = acc / (float)a.Nout;
}

struct MmoeBwdArgs {
  const float* sv_exp;            // [M, H E]
  const float* sv_gate;           // [M, T E]
  const float* sv_a[MMOE_MAXL];   // a_l [M, T N_l], l < L-1
  float* deltas[MMOE_MAXL];       // delta_l, the same layout
  const float* G;                 // [M, T Nout], rows Gs apart
  int64_t Gs;
  const float* prep;
  int d, dp, H, Hp, E, T, L, N1, N1p, rs, unroll, Nout;
  int K[MMOE_MAXL], Kp[MMOE_MAXL], Np[MMOE_MAXL], act[MMOE_MAXL];
  int64_t woff[MMOE_MAXL], w1off;
  float* dz1;  // [M, N1], rows dz1s apart
  int64_t dz1s;
  float* dx;   // [M, d], rows dxs apart, or null
  int64_t dxs;
  int64_t M;
};

template <int NW>
__global__ __launch_bounds__(NW * 64) void mmoe_bwd(MmoeBwdArgs a) {
  extern __shared__ float smem[];
  const int RS = a.rs;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t m0 = (int64_t)blockIdx.x * 16;
  const int HE = a.H * a.E, TE = a.T * a.E, LT = a.L - 1;
  float* bufC = smem + 32 * RS;  // [relu experts | gates], stage-1 column order
  float* red = smem + 48 * RS;

  // the top layer's weights first, then the tile's G, experts and gates, one
  // row per wave
  floatx4 ring[MLP_R];
  auto fill_chain = [&](int l) {
    mmoe_first_fill<NW>(a.prep + a.woff[l], a.T * (a.Kp[l] >> 4), a.Np[l] >> 4, ring);
  };
  fill_chain(LT);
  for (int r = w; r < 16; r += NW) {
    const int64_t m = m0 + r < a.M ? m0 + r : a.M - 1;
    const int Np = a.Np[LT];
    for (int c = lane; c < a.T * Np; c += 64) {
      const int t = c / Np, j = c - t * Np;
      smem[r * RS + c] = j < a.Nout ? a.G[m * a.Gs + t * a.Nout + j] : 0.f;
    }
    for (int c = lane; c < a.N1; c += 64)
      bufC[r * RS + c] = c < HE ? a.sv_exp[m * HE + c] : a.sv_gate[m * TE + (c - HE)];
  }

  // ---- the towers, top down: layer l of every task as one layer
  float* in = smem;
  float* out = smem + 16 * RS;
  for (int l = LT; l >= 0; --l) {
    const int Tl = a.Kp[l] >> 4, Kp = a.Kp[l], Np = a.Np[l], Nk = a.K[l];
    const bool relu = l > 0 && a.act[l - 1] == RS_ACT_RELU;
    const float* mk = l > 0 ? a.sv_a[l - 1] : nullptr;
    float* dl = l > 0 ? a.deltas[l - 1] : nullptr;
    __syncthreads();  // the layer's input complete
    mmoe_layer<NW, false>(
        a.prep + a.woff[l], nullptr, a.T * Tl, Np >> 4, in, RS, red, ring, a.unroll,
        [&](int tt) { return (tt / Tl) * Np; },
        [&](int row, int col, float v, float) {
          if (l > 0) {
            const int t = col / Kp, k = col - t * Kp;
            const int64_t m = m0 + row;
            if (k < Nk) {  // (padded columns: exact zeros from the zero weights)
              const int64_t at = ((m < a.M ? m : a.M - 1) * a.T + t) * Nk + k;
              if (relu) v = mk[at] > 0.f ? v : 0.f;
              if (m < a.M) dl[at] = v;
            }
          }
          out[row * RS + col] = v;
        },
        [&] {
          if (l > 0) fill_chain(l - 1);
          else if (a.dx) mmoe_first_fill<NW>(a.prep + a.w1off, a.dp >> 4, a.N1p >> 4, ring);
        });
    float* tmp = in;
    in = out;
    out = tmp;
  }
  const float* dm = in;  // dmix [16][t Hp + h]
  float* dz = out;       // dz1 [16][N1p]

  // ---- gates: dp_t[e] = sum_h dmix_t[h] expert[h, e], h ascending
  __syncthreads();  // dmix complete
  for (int i = threadIdx.x; i < 16 * TE; i += NW * 64) {
    const int row = i / TE, q = i - row * TE, t = q / a.E, e = q - t * a.E;
    const float* dmr = dm + row * RS + t * a.Hp;
    const float* er = bufC + row * RS + e;
    float s = 0.f;
    for (int h = 0; h < a.H; ++h) s = fmaf(dmr[h], er[h * a.E], s);
    red[i] = s;
  }
  __syncthreads();  // dp complete
  for (int i = threadIdx.x; i < 16 * TE; i += NW * 64) {
    const int row = i / TE, q = i - row * TE, t = q / a.E, e = q - t * a.E;
    const float* pr = bufC + row * RS + HE + t * a.E;
    const float* dpr = red + row * TE + t * a.E;
    float s = 0.f;
    for (int e2 = 0; e2 < a.E; ++e2) s = fmaf(pr[e2], dpr[e2], s);
    const float v = pr[e] * (dpr[e] - s);
    dz[row * RS + HE + q] = v;
    const int64_t m = m0 + row;
    if (m < a.M) a.dz1[m * a.dz1s + HE + q] = v;
  }
  // ---- experts: dexp[h, e] = [expert > 0] sum_t p_t[e] dmix_t[h], t ascending
  for (int i = threadIdx.x; i < 16 * HE; i += NW * 64) {
    const int row = i / HE, c = i - row * HE, h = c / a.E, e = c - h * a.E;
    const float* pr = bufC + row * RS + HE + e;
    const float* dmr = dm + row * RS + h;
    float s = 0.f;
    for (int t = 0; t < a.T; ++t) s = fmaf(pr[t * a.E], dmr[t * a.Hp], s);
    const float v = bufC[row * RS + c] > 0.f ? s : 0.f;
    dz[row * RS + c] = v;
    const int64_t m = m0 + row;
    if (m < a.M) a.dz1[m * a.dz1s + c] = v;
  }
  if (!a.dx) return;  // (uniform)
  const int pad = a.N1p - a.N1;
  for (int i = threadIdx.x; i < 16 * pad; i += NW * 64) dz[(i / pad) * RS + a.N1 + i % pad] = 0.f;

  // ---- dx = dz1 W1^T
  __syncthreads();  // dz1 complete; dp (red) no longer read
  mmoe_layer<NW, false>(
      a.prep + a.w1off, nullptr, a.dp >> 4, a.N1p >> 4, dz, RS, red, ring, a.unroll, [](int) { return 0; },
      [&](int row, int col, float v, float) {
        const int64_t m = m0 + row;
        if (m < a.M && col < a.d) a.dx[m * a.dxs + col] = v;
      },
      [] {});
}

}  // namespace rs

using namespace rs;

#define MMOE_TRAIN_SHAPE_MSG \
  "need a shape rs_mmoe_ok takes with 1..%d tower layers whose backward tile (three LDS tiles) fits the LDS"

extern "C" int rs_mmoe_train_ok(int d, int hidden, int n_experts, int n_tasks, int n_tower_layers,
                                const int* tower_dims) {
  MmoeTrainGeom g;
  return mmoe_train_geom(d, hidden, n_experts, n_tasks, n_tower_layers, tower_dims, g) ? 1 : 0;
}

extern "C" int64_t rs_mmoe_saved_size(int d, int hidden, int n_experts, int n_tasks, int n_tower_layers,
                                      const int* tower_dims, int64_t batch) {
  MmoeTrainGeom g;
  if (batch < 0 || !mmoe_train_geom(d, hidden, n_experts, n_tasks, n_tower_layers, tower_dims, g)) {
    set_error("rs_mmoe_saved_size: batch >= 0; " MMOE_TRAIN_SHAPE_MSG, MMOE_MAXL);
    return -1;
  }
  return batch * mmoe_saved(g.f).per;
}

// the hidden activations the backward takes: relu or none, a linear output
static bool mmoe_train_acts(const int* acts, int L) {
  if (!acts || acts[L - 1] != RS_ACT_NONE) return false;
  for (int l = 0; l + 1 < L; ++l)
    if (acts[l] != RS_ACT_NONE && acts[l] != RS_ACT_RELU) return false;
  return true;
}
#define MMOE_TRAIN_ACT_MSG "tower activations: relu or none on the hidden layers, none on the output layer"

extern "C" int rs_mmoe_train_fwd(const float* x, int64_t x_stride, int d, int hidden, int n_experts, int n_tasks,
                                 int n_tower_layers, const int* tower_dims, const int* tower_acts,
                                 const float* prepared, float* saved, float* y, int64_t y_task_stride,
                                 int64_t y_stride, int64_t batch, rs_stream_t stream) {
  if (batch == 0) return RS_OK;
  MmoeTrainGeom g;
  RS_REQUIRE(mmoe_train_geom(d, hidden, n_experts, n_tasks, n_tower_layers, tower_dims, g),
             "rs_mmoe_train_fwd: " MMOE_TRAIN_SHAPE_MSG, MMOE_MAXL);
  RS_REQUIRE(saved, "rs_mmoe_train_fwd: null pointer (saved)");
  RS_REQUIRE(mmoe_train_acts(tower_acts, g.f.L), "rs_mmoe_train_fwd: " MMOE_TRAIN_ACT_MSG);
  return mmoe_fwd_run<true>("rs_mmoe_train_fwd", x, x_stride, d, hidden, n_experts, n_tasks, n_tower_layers,
                            tower_dims, tower_acts, prepared, nullptr, 0, y, y_task_stride, y_stride, saved, batch,
                            stream);
}

extern "C" int rs_mmoe_head_grad(const float* z, int64_t z_task_stride, int64_t z_stride, const float* labels,
                                 int64_t labels_task_stride, int64_t labels_stride, const float* loss_weights,
                                 int n_out, int n_tasks, int64_t batch, float* G, int64_t G_stride, float* loss,
                                 rs_stream_t stream) {
  if (batch == 0) return RS_OK;
  RS_REQUIRE(n_out >= 1 && n_out <= MLP_MAXD && n_tasks >= 1 && n_tasks <= MMOE_MAXT && batch > 0,
             "rs_mmoe_head_grad: need 1..%d outputs, 1..%d tasks, batch >= 0", MLP_MAXD, MMOE_MAXT);
  RS_REQUIRE(z && labels && G, "rs_mmoe_head_grad: null pointer (z, labels, G)");
  RS_REQUIRE(z_stride >= n_out && z_task_stride >= n_out && labels_stride >= n_out && labels_task_stride >= n_out,
             "rs_mmoe_head_grad: z / labels stride smaller than the output width");
  RS_REQUIRE(G_stride >= (int64_t)n_tasks * n_out, "rs_mmoe_head_grad: G_stride smaller than n_tasks * n_out");
  const int64_t n = batch * n_tasks, grid = (n + 255) / 256;
  RS_REQUIRE(grid < (1ll << 31), "rs_mmoe_head_grad: batch too large");
  MmoeHeadArgs a{};
  a.z = z;
  a.zts = z_task_stride;
  a.zs = z_stride;
  a.y = labels;
  a.yts = labels_task_stride;
  a.ys = labels_stride;
  for (int t = 0; t < n_tasks; ++t) a.w[t] = loss_weights ? loss_weights[t] : 1.0f;
  a.Nout = n_out;
  a.T = n_tasks;
  a.M = batch;
  a.G = G;
  a.Gs = G_stride;
  a.loss = loss;
  mmoe_head_grad<<<(unsigned)grid, 256, 0, as_stream(stream)>>>(a);
  return launch_status("rs_mmoe_head_grad");
}

extern "C" int64_t rs_mmoe_bwd_prepared_size(int d, int hidden, int n_experts, int n_tasks, int n_tower_layers,
                                             const int* tower_dims) {
  MmoeTrainGeom g;
  if (!mmoe_train_geom(d, hidden, n_experts, n_tasks, n_tower_layers, tower_dims, g)) {
    set_error("rs_mmoe_bwd_prepared_size: " MMOE_TRAIN_SHAPE_MSG, MMOE_MAXL);
    return -1;
  }
  return g.total;
}

extern "C" int rs_mmoe_prepare_bwd(int d, int hidden, int n_experts, int n_tasks, const float* expert_matrix,
                                   const float* const* gate_matrix, int n_tower_layers, const int* tower_dims,
                                   const float* const* tower_W, float* prepared_bwd, rs_stream_t stream) {
  MmoeTrainGeom g;
  RS_REQUIRE(mmoe_train_geom(d, hidden, n_experts, n_tasks, n_tower_layers, tower_dims, g),
             "rs_mmoe_prepare_bwd: " MMOE_TRAIN_SHAPE_MSG, MMOE_MAXL);
  const MmoeGeom& f = g.f;
  RS_REQUIRE(expert_matrix && gate_matrix && tower_W && prepared_bwd, "rs_mmoe_prepare_bwd: null pointer");
  for (int t = 0; t < f.T; ++t) RS_REQUIRE(gate_matrix[t], "rs_mmoe_prepare_bwd: task %d has no gate_matrix", t);
  for (int i = 0; i < f.T * f.L; ++i)
    RS_REQUIRE(tower_W[i], "rs_mmoe_prepare_bwd: task %d tower layer %d has no kernel", i / f.L, i % f.L);
  for (int l = 0; l < f.L; ++l) {
    MmoePrepBwdLayerArgs q{};
    for (int t = 0; t < f.T; ++t) q.W[t] = tower_W[t * f.L + l];
    q.K = f.K[l];
    q.N = f.N[l];
    q.Kp = f.Kp[l];
    q.Np = f.Np[l];
    q.T = f.T;
    q.out = prepared_bwd + g.woff[l];
    const int64_t n = (int64_t)f.T * f.Kp[l] * f.Np[l];
    mmoe_prepare_bwd_layer<<<(unsigned)((n + 255) / 256), 256, 0, as_stream(stream)>>>(q);
  }
  MmoePrepBwd1Args p{};
  p.ew = expert_matrix;
  for (int t = 0; t < f.T; ++t) p.gw[t] = gate_matrix[t];
  p.d = f.d;
  p.dp = f.dp;
  p.HE = f.H * f.E;
  p.E = f.E;
  p.N1 = f.N1;
  p.N1p = f.N1p;
  p.out = prepared_bwd + g.w1off;
  const int64_t n1 = (int64_t)f.N1p * f.dp;
  mmoe_prepare_bwd_stage1<<<(unsigned)((n1 + 255) / 256), 256, 0, as_stream(stream)>>>(p);
  return launch_status("rs_mmoe_prepare_bwd");
}

extern "C" int rs_mmoe_bwd(const float* saved, const float* G, int64_t G_stride, int d, int hidden, int n_experts,
                           int n_tasks, int n_tower_layers, const int* tower_dims, const int* tower_acts,
                           const float* prepared_bwd, float* deltas, float* dz1, int64_t dz1_stride, float* dx,
                           int64_t dx_stride, int64_t batch, rs_stream_t stream) {
  if (batch == 0) return RS_OK;
  MmoeTrainGeom g;
  RS_REQUIRE(mmoe_train_geom(d, hidden, n_experts, n_tasks, n_tower_layers, tower_dims, g),
             "rs_mmoe_bwd: " MMOE_TRAIN_SHAPE_MSG, MMOE_MAXL);
  const MmoeGeom& f = g.f;
  RS_REQUIRE(saved && G && prepared_bwd && dz1, "rs_mmoe_bwd: null pointer (saved, G, prepared_bwd, dz1)");
  RS_REQUIRE(f.L == 1 || deltas, "rs_mmoe_bwd: null pointer (deltas, with hidden tower layers)");
  RS_REQUIRE(mmoe_train_acts(tower_acts, f.L), "rs_mmoe_bwd: " MMOE_TRAIN_ACT_MSG);
  const int Nout = f.N[f.L - 1];
  RS_REQUIRE(batch > 0 && G_stride >= (int64_t)f.T * Nout, "rs_mmoe_bwd: bad batch/stride (G_stride < n_tasks * n_out)");
  RS_REQUIRE(dz1_stride >= f.N1, "rs_mmoe_bwd: dz1_stride smaller than (hidden + n_tasks) * n_experts");
  RS_REQUIRE(!dx || dx_stride >= d, "rs_mmoe_bwd: dx_stride smaller than d");
  const int64_t grid = (batch + 15) / 16;
  RS_REQUIRE(grid < (1ll << 31), "rs_mmoe_bwd: batch too large");
  const MmoeSaved s = mmoe_saved(f);
  MmoeBwdArgs a{};
  a.sv_exp = saved;
  a.sv_gate = saved + batch * s.gate;
  for (int l = 0; l + 1 < f.L; ++l) {
    a.sv_a[l] = saved + batch * s.a[l];
    a.deltas[l] = deltas + batch * (s.a[l] - s.a[0]);
  }
  a.G = G;
  a.Gs = G_stride;
  a.prep = prepared_bwd;
  a.d = f.d;
  a.dp = f.dp;
  a.H = f.H;
  a.Hp = f.Hp;
  a.E = f.E;
  a.T = f.T;
  a.L = f.L;
  a.N1 = f.N1;
  a.N1p = f.N1p;
  a.rs = g.rs;
  a.unroll = opt(RS_OPT_MLP_UNROLL);
  a.Nout = Nout;
  for (int l = 0; l < f.L; ++l) {
    a.K[l] = f.K[l];
    a.Kp[l] = f.Kp[l];
    a.Np[l] = f.Np[l];
    a.act[l] = tower_acts[l];
    a.woff[l] = g.woff[l];
  }
  a.w1off = g.w1off;
  a.dz1 = dz1;
  a.dz1s = dz1_stride;
  a.dx = dx;
  a.dxs = dx_stride;
  a.M = batch;
  launch_lds<mmoe_bwd<MMOE_NW>>((unsigned)grid, MMOE_NW * 64, g.lds, as_stream(stream), a);
  return launch_status("rs_mmoe_bwd");
}
