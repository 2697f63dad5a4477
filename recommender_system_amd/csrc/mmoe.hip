// mmoe.hip — the multi-gate mixture-of-experts forward in one launch:
// mmoe_layer.call (layer/interaction.py:479-509: E experts x @ expert_matrix
// [:, :, e] (+ expert_bias, relu), per task a softmax gate x @ gate_matrix_t
// (+ gate_bias_t), the gated sum over the experts) and the T towers of
// MMOE.call (model/mmoe.py:24-32: tower_layer, layer/interaction.py:512-523,
// Dense(h_i, act) per hidden width then a linear Dense(output_dim), task t's
// tower on task t's mix).
//
// Layout and schedule (gfx950), on the fused MLP tower's machinery
// (mlp_tower.hpp: B-fragment packing, weight ring, tile x k-slice work split
// with its fixed-order reduction):
//   * A workgroup owns 16 samples and 16 waves; two LDS tiles [16][rs] and the
//     partial-tile area of the K-split.  No intermediate touches HBM.
//   * Stage 1.  x [16, d] is staged once (buf0) and contracted with ONE packed
//     matrix of N1 = H E + T E columns: column h E + e = expert_matrix[:, h, e]
//     (the Keras tensor [d, H, E] read as [d, H E]; relu), column H E + t E + e
//     = gate_matrix_t[:, e] (linear).  The result z goes to buf1 TRANSPOSED per
//     expert: expert (h, e) at column e Hs + h with Hs = H | 1, task t's gate
//     logits at E Hs + t E.  The mix below then reads consecutive h from
//     consecutive lanes (conflict-free ds_read_b32); read where the contraction
//     leaves them (lanes E floats apart) E = 8 / 16 would put 8 / 16 lanes of a
//     half-wave on one bank.  Hs odd keeps the transposing store's e-stride off
//     the banks' period.  The columns that pad N1 up to 16 are never stored.
//   * Stage 2.  One thread per (row, task, h): the softmax of the task's E
//     gate logits (maximum subtracted, the sum in ascending e; recomputed per h
//     — E <= 16 exponentials — which saves a barrier against a separate gate
//     pass), then mix = sum_e (p_e / s) z[e Hs + h] in ascending e, written to
//     buf0 at column t Hp + h (Hp = roundup(H, 16); the pad columns are zeroed)
//     and, when asked for, to mix [B, T H].
//   * Stage 3.  Tower layer l of ALL tasks is one block-diagonal layer: its
//     work items are (task, output tile, k-slice) over T Np_l / 16 tiles — the
//     packed image of a layer is the tasks' packed kernels one after another,
//     so item (task, tile) is tile task Np_l / 16 + tile of one matrix whose A
//     fragment starts at column task Kp_l — with one barrier per layer (two
//     when the k-slices meet in LDS), not T serial chains.
//   * Biases are read from the packed image (L2) by the finishing lane, the
//     load in flight over the contraction.
//   * Every sum has one fixed order; a row's result does not depend on the
//     batch or on the row's place in its tile.  Rows past the batch re-read the
//     last row and are never stored.
// The device side (geometry, the block-diagonal layer, the kernel) lives in
// mmoe.hpp, shared with the training entries (mmoe_train.hip); this file holds
// the prepare kernels and the forward's entry points.
#include "mmoe.hpp"

namespace rs {

struct MmoePrep1Args {
  const float* ew;  // [d, H E]
  const float* eb;  // [H E] or null
  const float* gw[MMOE_MAXT];  // [d, E]
  const float* gb[MMOE_MAXT];  // [E] or null
  int d, dp, HE, E, N1, N1p;
  float* out;
};

__global__ void mmoe_prepare_stage1(MmoePrep1Args a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nw = (int64_t)a.dp * a.N1p;
  if (i >= nw + a.N1p) return;
  float v = 0.f;
  if (i < nw) {
    int k, n;
    mmoe_unpack(i, a.dp / 16, k, n);
    if (k < a.d && n < a.HE) {
      v = a.ew[(int64_t)k * a.HE + n];
    } else if (k < a.d && n < a.N1) {
      const int t = (n - a.HE) / a.E, e = (n - a.HE) - t * a.E;
      v = a.gw[t][(int64_t)k * a.E + e];
    }
  } else {
    const int n = (int)(i - nw);
    if (n < a.HE) {
      v = a.eb ? a.eb[n] : 0.f;
    } else if (n < a.N1) {
      const int t = (n - a.HE) / a.E, e = (n - a.HE) - t * a.E;
      v = a.gb[t] ? a.gb[t][e] : 0.f;
    }
  }
  a.out[i] = v;
}

struct MmoePrepLayerArgs {
  const float* W[MMOE_MAXT];     // task t's kernel [K, N]
  const float* bias[MMOE_MAXT];  // [N] or null
  int K, N, Kp, Np, T;
  float* out;
};

__global__ void mmoe_prepare_layer(MmoePrepLayerArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t per = (int64_t)a.Kp * a.Np, nw = per * a.T;
  if (i >= nw + (int64_t)a.T * a.Np) return;
  float v = 0.f;
  if (i < nw) {
    const int t = (int)(i / per);
    int k, n;
    mmoe_unpack(i - t * per, a.Kp / 16, k, n);
    if (k < a.K && n < a.N) v = a.W[t][(int64_t)k * a.N + n];
  } else {
    const int q = (int)(i - nw), t = q / a.Np, n = q - t * a.Np;
    if (n < a.N && a.bias[t]) v = a.bias[t][n];
  }
  a.out[i] = v;
}

}  // namespace rs

using namespace rs;

extern "C" int rs_mmoe_ok(int d, int hidden, int n_experts, int n_tasks, int n_tower_layers, const int* tower_dims) {
  MmoeGeom g;
  return mmoe_geom(d, hidden, n_experts, n_tasks, n_tower_layers, tower_dims, g) ? 1 : 0;
}

extern "C" int64_t rs_mmoe_prepared_size(int d, int hidden, int n_experts, int n_tasks, int n_tower_layers,
                                         const int* tower_dims) {
  MmoeGeom g;
  if (!mmoe_geom(d, hidden, n_experts, n_tasks, n_tower_layers, tower_dims, g)) {
    set_error("rs_mmoe_prepared_size: " MMOE_SHAPE_MSG, MMOE_SHAPE_ARGS);
    return -1;
  }
  return g.total;
}

extern "C" int rs_mmoe_prepare(int d, int hidden, int n_experts, int n_tasks, const float* expert_matrix,
                               const float* expert_bias, const float* const* gate_matrix,
                               const float* const* gate_bias, int n_tower_layers, const int* tower_dims,
                               const float* const* tower_W, const float* const* tower_bias, float* prepared,
                               rs_stream_t stream) {
  MmoeGeom g;
  RS_REQUIRE(mmoe_geom(d, hidden, n_experts, n_tasks, n_tower_layers, tower_dims, g),
             "rs_mmoe_prepare: " MMOE_SHAPE_MSG, MMOE_SHAPE_ARGS);
  RS_REQUIRE(expert_matrix && gate_matrix && prepared && (g.L == 0 || tower_W), "rs_mmoe_prepare: null pointer");
  for (int t = 0; t < g.T; ++t) RS_REQUIRE(gate_matrix[t], "rs_mmoe_prepare: task %d has no gate_matrix", t);
  for (int i = 0; i < g.T * g.L; ++i)
    RS_REQUIRE(tower_W[i], "rs_mmoe_prepare: task %d tower layer %d has no kernel", i / g.L, i % g.L);
  MmoePrep1Args p{};
  p.ew = expert_matrix;
  p.eb = expert_bias;
  for (int t = 0; t < g.T; ++t) {
    p.gw[t] = gate_matrix[t];
    p.gb[t] = gate_bias ? gate_bias[t] : nullptr;
  }
  p.d = g.d;
  p.dp = g.dp;
  p.HE = g.H * g.E;
  p.E = g.E;
  p.N1 = g.N1;
  p.N1p = g.N1p;
  p.out = prepared;
  const int64_t n1 = g.b1off + g.N1p;
  mmoe_prepare_stage1<<<(unsigned)((n1 + 255) / 256), 256, 0, as_stream(stream)>>>(p);
  for (int l = 0; l < g.L; ++l) {
    MmoePrepLayerArgs q{};
    for (int t = 0; t < g.T; ++t) {
      q.W[t] = tower_W[t * g.L + l];
      q.bias[t] = tower_bias ? tower_bias[t * g.L + l] : nullptr;
    }
    q.K = g.K[l];
    q.N = g.N[l];
    q.Kp = g.Kp[l];
    q.Np = g.Np[l];
    q.T = g.T;
    q.out = prepared + g.off[l];
    const int64_t n = (int64_t)g.T * g.Np[l] * (g.Kp[l] + 1);
    mmoe_prepare_layer<<<(unsigned)((n + 255) / 256), 256, 0, as_stream(stream)>>>(q);
  }
  return launch_status("rs_mmoe_prepare");
}

extern "C" int rs_mmoe_fwd(const float* x, int64_t x_stride, int d, int hidden, int n_experts, int n_tasks,
                           int n_tower_layers, const int* tower_dims, const int* tower_acts, const float* prepared,
                           float* mix, int64_t mix_stride, float* y, int64_t y_task_stride, int64_t y_stride,
                           int64_t batch, rs_stream_t stream) {
  if (batch == 0) return RS_OK;  // empty batch: nothing to launch (null data pointers allowed)
  return mmoe_fwd_run<false>("rs_mmoe_fwd", x, x_stride, d, hidden, n_experts, n_tasks, n_tower_layers, tower_dims,
                             tower_acts, prepared, mix, mix_stride, y, y_task_stride, y_stride, nullptr, batch,
                             stream);
}
