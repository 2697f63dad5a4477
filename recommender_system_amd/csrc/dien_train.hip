// dien_train.hip — training of DIEN's two recurrences (dien_rnn.hpp):
//   * rs_gru_train_fwd / rs_augru_train_fwd: dien_rnn<., SAVE>, the forwards of
//     dien.hip (the same device functions, so seq / last are bit-identical)
//     that also store per step what the backward reads:
//       GRU    saved[b][t] = z | r | hh | hr_h | h_prev     (5 x Up floats)
//       AUGRU  saved[b][t] = u | r | hh | h_prev            (4 x Up floats)
//     with u = hsig(a_z), r = hsig(a_r); z = a u is recomputed from the score.
//   * rs_gru_bwd / rs_augru_bwd: backpropagation through time, t = T-1 .. 0,
//     one workgroup per 16-sample tile, wave c owning units 16 c .. 16 c + 15
//     of all gates as in the forward.  Only the h -> h chain is in the loop:
//       GRU    dh_prev = dh z + [da_z, da_r, dc r] U^T          one barrier
//       AUGRU  d(rh) = dc U_h^T, then                            two barriers
//              dh_prev = keep + d(rh) r + [da_z, da_r] U_zr^T
//     The gate gradients go through LDS once per dependent matmul (rotated
//     [16][Up] tiles, dn_off), dh stays in registers, and the transposed
//     recurrent kernel (rs_gru_prepare_bwd: fragment (gate, c, g), lane l,
//     element j = U[16 c + (l & 15)][gate units + 16 g + 4 (l >> 4) + j]) stays
//     in registers for the whole loop.  A column of the MFMA is a sample: no
//     per-sample result depends on tile mates or the batch.  Saved planes and
//     upstream gradients of step t - 1 are loaded before step t's barrier.
//   * Off the chain the kernels write the operands of the weight gradients as
//     [B T, .] matrices (gx, gh, h_prev | r h_prev); dW, dU, dx and the bias
//     gradients are rs_gemm / rs_col_sum_split at M = B T on the host side.
//   * rs_augru_bwd also reduces da[b, t] = sum_units dz u (quad shuffles, then
//     the waves' partials in wave order through LDS) and applies the masked
//     softmax's backward per sample in t order.
#include "dien_rnn.hpp"

namespace rs {

// U [units, 3 units] -> 3 gates x Up/16 tiles x Up/16 k-groups x 64 lanes x 4 of U^T
__global__ void dien_pack_t(const float* U, int units, int Up, float* out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 3ll * Up * Up) return;
  const int j = (int)(i & 3), lane = (int)((i >> 2) & 63);
  const int blk = (int)(i >> 8), G = Up / 16;
  const int g = blk % G, tt = blk / G, gate = tt / G, c = tt - gate * G;
  const int v = 16 * g + 4 * (lane >> 4) + j, u = 16 * c + (lane & 15);
  out[i] = v < units && u < units ? U[(int64_t)u * 3 * units + gate * units + v] : 0.f;
}

struct RnnBwdArgs {
  const float* saved;
  const float* scores;  // AUGRU: [B, T], rows ssb apart
  int64_t ssb;
  const void* len;
  int len_kind, norm, paper;
  const float* dseq;   // GRU: [B, T, U] or null
  const float* dlast;  // [B, U], rows dls apart (GRU: or null)
  int64_t dls;
  const float* prep;  // rs_gru_prepare_bwd
  int T, U, Up, G;
  float* gx;  // [B T, 3 U]
  float* gh;  // GRU: [B T, 3 U]
  float* hp;  // GRU: h_prev [B T, U]; AUGRU: [h_prev | r h_prev] [B T, 2 U]
  float* ds;  // AUGRU: [B, T]
  float* da;  // AUGRU: [B, T] or null
  int64_t M;
};

__device__ __forceinline__ int64_t dt_len(const void* len, int kind, int64_t b) {
  return kind == RS_ID_I64 ? static_cast<const int64_t*>(len)[b] : (int64_t) static_cast<const int32_t*>(len)[b];
}
// acc += Ut_gate^T tile^T over G k-groups (tile: a rotated [16][Up] LDS tile)
__device__ __forceinline__ floatx4 dt_mac(const floatx4 (&Ut)[DN_MAXG], int G, const float* tile,
                                          const int (&aoff)[DN_MAXG], floatx4 acc) {
#pragma unroll
  for (int g = 0; g < DN_MAXG; ++g) {
    if (g < G) {
      const floatx4 x = *reinterpret_cast<const floatx4*>(tile + aoff[g]);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = mfma16x16x4(Ut[g][j], x[j], acc);
    }
  }
  return acc;
}
// four units of a [rows, ld] matrix at column col0 + r, units past U skipped
__device__ __forceinline__ void dt_store(float* m, int64_t row, int64_t ld, int col0, int u, int U, const floatx4& v) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (u + r < U) m[row * ld + col0 + u + r] = v[r];
}
__device__ __forceinline__ floatx4 dt_load(const float* m, int64_t off, int u, int U) {
  floatx4 v;
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = m && u + r < U ? m[off + u + r] : 0.f;
  return v;
}

__global__ __launch_bounds__(DN_MAXG * 64) void dien_gru_bwd(RnnBwdArgs a) {
  __shared__ float gb[2][3][16 * 16 * DN_MAXG];
  const int T = a.T, U = a.U, Up = a.Up, G = a.G, NC = 4 * G;
  const int lane = threadIdx.x & 63;
  const int c = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int s = lane & 15, kk = lane >> 4;
  const int64_t m0 = (int64_t)blockIdx.x * 16;
  const int64_t mrow = m0 + s < a.M ? m0 + s : a.M - 1;  // rows past the batch repeat the last row, never stored
  const bool live = m0 + s < a.M, mine = c < G;
  const int u = 16 * c + 4 * kk;
  const floatx4 zero = {0.f, 0.f, 0.f, 0.f};
  floatx4 Ut[3][DN_MAXG];
  int aoff[DN_MAXG];
  int hoff = 0;
  if (mine) {
    dn_load_w(a.prep, c, G, G, Ut);
#pragma unroll
    for (int g = 0; g < DN_MAXG; ++g) aoff[g] = dn_off(s, 4 * g + kk, NC);
    hoff = dn_off(s, 4 * c + kk, NC);
  }
  auto plane = [&](int t, int p) {
    return *reinterpret_cast<const floatx4*>(a.saved + ((mrow * T + t) * DN_GRU_PLANES + p) * Up + u);
  };
  // the upstream gradient of h_t that does not come through the chain
  auto upstream = [&](int t) {
    floatx4 g = dt_load(a.dseq, (mrow * T + t) * U, u, U);
    if (t == T - 1) g += dt_load(a.dlast, mrow * a.dls, u, U);
    return g;
  };
  floatx4 z = zero, rg = zero, hh = zero, hrh = zero, h0 = zero, up = zero, dh = zero;
  if (mine) {
    z = plane(T - 1, 0), rg = plane(T - 1, 1), hh = plane(T - 1, 2), hrh = plane(T - 1, 3), h0 = plane(T - 1, 4);
    up = upstream(T - 1);
  }
  for (int t = T - 1; t >= 0; --t) {
    floatx4 keep = zero;
    if (mine) {
      floatx4 daz, dar, dc, dcr;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float d = dh[r] + up[r];
        const float dz = d * (h0[r] - hh[r]);
        const float dhh = d * (1.0f - z[r]);
        dc[r] = dhh * (1.0f - hh[r] * hh[r]);
        daz[r] = dz * z[r] * (1.0f - z[r]);
        dar[r] = dc[r] * hrh[r] * rg[r] * (1.0f - rg[r]);
        dcr[r] = dc[r] * rg[r];
        keep[r] = d * z[r];
      }
      float* tile = gb[t & 1][0];
      *reinterpret_cast<floatx4*>(tile + hoff) = daz;
      *reinterpret_cast<floatx4*>(tile + 16 * 16 * DN_MAXG + hoff) = dar;
      *reinterpret_cast<floatx4*>(tile + 2 * 16 * 16 * DN_MAXG + hoff) = dcr;
      if (live) {
        const int64_t row = (m0 + s) * T + t;
        dt_store(a.gx, row, 3 * U, 0, u, U, daz);
        dt_store(a.gx, row, 3 * U, U, u, U, dar);
        dt_store(a.gx, row, 3 * U, 2 * U, u, U, dc);
        dt_store(a.gh, row, 3 * U, 0, u, U, daz);
        dt_store(a.gh, row, 3 * U, U, u, U, dar);
        dt_store(a.gh, row, 3 * U, 2 * U, u, U, dcr);
        dt_store(a.hp, row, U, 0, u, U, h0);
      }
      if (t > 0) {  // off the chain: in flight while the waves arrive
        z = plane(t - 1, 0), rg = plane(t - 1, 1), hh = plane(t - 1, 2), hrh = plane(t - 1, 3), h0 = plane(t - 1, 4);
        up = upstream(t - 1);
      }
    }
    __syncthreads();  // the three gate-gradient tiles of step t complete
    if (mine && t > 0) {
      const float* tile = gb[t & 1][0];
      const floatx4 a0 = dt_mac(Ut[0], G, tile, aoff, keep);
      const floatx4 a1 = dt_mac(Ut[1], G, tile + 16 * 16 * DN_MAXG, aoff, zero);
      const floatx4 a2 = dt_mac(Ut[2], G, tile + 2 * 16 * 16 * DN_MAXG, aoff, zero);
      dh = (a0 + a1) + a2;
    }
  }
}

__device__ __forceinline__ float dt_slope(float v) { return v > 0.f && v < 1.f ? 0.2f : 0.f; }

__global__ __launch_bounds__(DN_MAXG * 64) void dien_augru_bwd(RnnBwdArgs a) {
  __shared__ float tb[3][16 * 16 * DN_MAXG];  // dc | da_z | da_r
  __shared__ float pda[DN_MAXG][16];
  const int T = a.T, U = a.U, Up = a.Up, G = a.G, NC = 4 * G;
  const int lane = threadIdx.x & 63;
  const int c = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int s = lane & 15, kk = lane >> 4;
  const int64_t m0 = (int64_t)blockIdx.x * 16;
  const int64_t mrow = m0 + s < a.M ? m0 + s : a.M - 1;
  const bool live = m0 + s < a.M, mine = c < G;
  const int u = 16 * c + 4 * kk;
  const floatx4 zero = {0.f, 0.f, 0.f, 0.f};
  floatx4 Ut[3][DN_MAXG];
  int aoff[DN_MAXG];
  int hoff = 0;
  if (mine) {
    dn_load_w(a.prep, c, G, G, Ut);
#pragma unroll
    for (int g = 0; g < DN_MAXG; ++g) aoff[g] = dn_off(s, 4 * g + kk, NC);
    hoff = dn_off(s, 4 * c + kk, NC);
  }
  auto plane = [&](int t, int p) {
    return *reinterpret_cast<const floatx4*>(a.saved + ((mrow * T + t) * DN_AUGRU_PLANES + p) * Up + u);
  };
  floatx4 uv = zero, rg = zero, hh = zero, h0 = zero, dh = zero;
  float at = 0.f;
  if (mine) {
    uv = plane(T - 1, 0), rg = plane(T - 1, 1), hh = plane(T - 1, 2), h0 = plane(T - 1, 3);
    at = a.scores[mrow * a.ssb + T - 1];
    dh = dt_load(a.dlast, mrow * a.dls, u, U);
  }
  for (int t = T - 1; t >= 0; --t) {
    floatx4 keep = zero, daz = zero, dc = zero;
    if (mine) {
      float part = 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float zz = at * uv[r], d = dh[r];
        float dz, dhh;
        if (a.paper) {
          dz = d * (hh[r] - h0[r]);
          keep[r] = d * (1.0f - zz);
          dhh = d * zz;
        } else {
          dz = d * (h0[r] - hh[r]);
          keep[r] = d * zz;
          dhh = d * (1.0f - zz);
        }
        dc[r] = dhh * (1.0f - hh[r] * hh[r]);
        daz[r] = dz * at * dt_slope(uv[r]);
        part += dz * uv[r];
      }
      *reinterpret_cast<floatx4*>(tb[0] + hoff) = dc;
      part += __shfl_xor(part, 16);
      part += __shfl_xor(part, 32);
      if (kk == 0) pda[c][s] = part;
    }
    __syncthreads();  // dc and the waves' parts of da complete
    if (mine) {
      const floatx4 drh = dt_mac(Ut[2], G, tb[0], aoff, zero);
      floatx4 dar, rh;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        dar[r] = drh[r] * h0[r] * dt_slope(rg[r]);
        keep[r] += drh[r] * rg[r];
        rh[r] = rg[r] * h0[r];
      }
      *reinterpret_cast<floatx4*>(tb[1] + hoff) = daz;
      *reinterpret_cast<floatx4*>(tb[2] + hoff) = dar;
      if (live) {
        const int64_t row = (m0 + s) * T + t;
        dt_store(a.gx, row, 3 * U, 0, u, U, daz);
        dt_store(a.gx, row, 3 * U, U, u, U, dar);
        dt_store(a.gx, row, 3 * U, 2 * U, u, U, dc);
        dt_store(a.hp, row, 2 * U, 0, u, U, h0);
        dt_store(a.hp, row, 2 * U, U, u, U, rh);
        if (c == 0 && kk == 0) {  // thread s: the same thread reads it back in the epilogue
          float v = pda[0][s];
          for (int w = 1; w < G; ++w) v += pda[w][s];
          a.ds[row] = v;
          if (a.da) a.da[row] = v;
        }
      }
      if (t > 0) {
        uv = plane(t - 1, 0), rg = plane(t - 1, 1), hh = plane(t - 1, 2), h0 = plane(t - 1, 3);
        at = a.scores[mrow * a.ssb + t - 1];
      }
    }
    __syncthreads();  // da_z, da_r complete (and pda, tb[0] free for step t - 1)
    if (mine && t > 0) {
      const floatx4 a0 = dt_mac(Ut[0], G, tb[1], aoff, keep);
      const floatx4 a1 = dt_mac(Ut[1], G, tb[2], aoff, zero);
      dh = a0 + a1;
    }
  }
  // ---- the masked softmax's backward: thread s < 16 wrote its sample's da
  // into ds above, and turns it into ds in place, t ascending
  if (threadIdx.x < 16 && live) {
    const int64_t L = dt_len(a.len, a.len_kind, m0 + s);
    float* row = a.ds + (m0 + s) * T;
    const float* p = a.scores + (m0 + s) * a.ssb;
    float dot = 0.f;
    if (a.norm)
      for (int t = 0; t < T; ++t)
        if (t < L) dot = fmaf(p[t], row[t], dot);
    for (int t = 0; t < T; ++t) row[t] = t < L ? (a.norm ? p[t] * (row[t] - dot) : row[t]) : 0.f;
  }
}

static int bwd_args(RnnBwdArgs& a, const char* what, const float* saved, int T, int units, const float* prepared_bwd,
                    int64_t batch) {
  GruGeom g;
  RS_REQUIRE(gru_geom(units, units, g), "%s: need 1 <= units <= %d", what, 16 * DN_MAXG);
  RS_REQUIRE(saved && prepared_bwd, "%s: null pointer (saved, prepared_bwd)", what);
  RS_REQUIRE(reinterpret_cast<uintptr_t>(saved) % 16 == 0, "%s: saved must be 16-byte aligned", what);
  RS_REQUIRE(T >= 1 && batch > 0, "%s: bad T / batch", what);
  RS_REQUIRE((batch + 15) / 16 < (1ll << 31) && batch * T < (1ll << 40), "%s: batch too large", what);
  a.saved = saved;
  a.prep = prepared_bwd;
  a.T = T;
  a.U = units;
  a.Up = g.Up;
  a.G = g.G;
  a.M = batch;
  return RS_OK;
}

static bool saved_size(int T, int din, int units, int64_t batch, int planes, int64_t& out) {
  GruGeom g;
  if (!gru_geom(din, units, g) || T < 1 || batch < 0 || batch * T >= (1ll << 40)) return false;
  out = batch * T * planes * g.Up;
  return true;
}

}  // namespace rs

using namespace rs;

extern "C" int64_t rs_gru_saved_size(int T, int din, int units, int64_t batch) {
  int64_t n;
  if (!saved_size(T, din, units, batch, DN_GRU_PLANES, n)) {
    set_error("rs_gru_saved_size: need T >= 1, batch >= 0 and 1 <= din, units <= %d", 16 * DN_MAXG);
    return -1;
  }
  return n;
}

extern "C" int64_t rs_augru_saved_size(int T, int din, int units, int64_t batch) {
  int64_t n;
  if (!saved_size(T, din, units, batch, DN_AUGRU_PLANES, n)) {
    set_error("rs_augru_saved_size: need T >= 1, batch >= 0 and 1 <= din, units <= %d", 16 * DN_MAXG);
    return -1;
  }
  return n;
}

extern "C" int64_t rs_gru_bwd_prepared_size(int units) {
  GruGeom g;
  if (!gru_geom(units, units, g)) {
    set_error("rs_gru_bwd_prepared_size: need 1 <= units <= %d", 16 * DN_MAXG);
    return -1;
  }
  return 3ll * g.Up * g.Up;
}

extern "C" int rs_gru_prepare_bwd(int units, const float* recurrent, float* prepared_bwd, rs_stream_t stream) {
  GruGeom g;
  RS_REQUIRE(gru_geom(units, units, g), "rs_gru_prepare_bwd: need 1 <= units <= %d", 16 * DN_MAXG);
  RS_REQUIRE(recurrent && prepared_bwd, "rs_gru_prepare_bwd: null pointer (recurrent, prepared_bwd)");
  const int64_t n = 3ll * g.Up * g.Up;
  dien_pack_t<<<(unsigned)((n + 255) / 256), 256, 0, as_stream(stream)>>>(recurrent, units, g.Up, prepared_bwd);
  return launch_status("rs_gru_prepare_bwd");
}

extern "C" int rs_gru_train_fwd(const float* x, int64_t x_bstride, int64_t x_tstride, int T, int din, int units,
                                const float* prepared, float* seq, float* last, int64_t last_stride, float* saved,
                                int64_t batch, rs_stream_t stream) {
  if (batch == 0) return RS_OK;
  RnnArgs a{};
  const int rc = rnn_args(a, "rs_gru_train_fwd", x, x_bstride, x_tstride, T, din, units, prepared, batch);
  if (rc != RS_OK) return rc;
  RS_REQUIRE(saved && reinterpret_cast<uintptr_t>(saved) % 16 == 0,
             "rs_gru_train_fwd: saved is null or not 16-byte aligned");
  RS_REQUIRE(seq || last, "rs_gru_train_fwd: null pointer (seq and last)");
  RS_REQUIRE(!last || last_stride >= units, "rs_gru_train_fwd: last_stride smaller than units");
  RS_REQUIRE(batch * T < (1ll << 40), "rs_gru_train_fwd: batch too large");
  a.seq = seq;
  a.last = last;
  a.ls = last_stride;
  a.saved = saved;
  dien_rnn<false, true><<<(unsigned)((batch + 15) / 16), DN_MAXG * 64, 0, as_stream(stream)>>>(a);
  return launch_status("rs_gru_train_fwd");
}

extern "C" int rs_augru_train_fwd(const float* x, int64_t x_bstride, int64_t x_tstride, const float* scores,
                                  int64_t scores_stride, int T, int din, int units, int augru_update,
                                  const float* prepared, float* last, int64_t last_stride, float* saved,
                                  int64_t batch, rs_stream_t stream) {
  if (batch == 0) return RS_OK;
  RnnArgs a{};
  const int rc = rnn_args(a, "rs_augru_train_fwd", x, x_bstride, x_tstride, T, din, units, prepared, batch);
  if (rc != RS_OK) return rc;
  RS_REQUIRE(scores && last, "rs_augru_train_fwd: null pointer (scores, last)");
  RS_REQUIRE(saved && reinterpret_cast<uintptr_t>(saved) % 16 == 0,
             "rs_augru_train_fwd: saved is null or not 16-byte aligned");
  RS_REQUIRE(scores_stride >= T && last_stride >= units, "rs_augru_train_fwd: bad scores_stride / last_stride");
  RS_REQUIRE(augru_update == 0 || augru_update == 1, "rs_augru_train_fwd: augru_update %d (0 reference, 1 paper)",
             augru_update);
  RS_REQUIRE(batch * T < (1ll << 40), "rs_augru_train_fwd: batch too large");
  a.scores = scores;
  a.ssb = scores_stride;
  a.paper = augru_update;
  a.last = last;
  a.ls = last_stride;
  a.saved = saved;
  dien_rnn<true, true><<<(unsigned)((batch + 15) / 16), DN_MAXG * 64, 0, as_stream(stream)>>>(a);
  return launch_status("rs_augru_train_fwd");
}

extern "C" int rs_gru_bwd(const float* saved, const float* dseq, const float* dlast, int64_t dlast_stride, int T,
                          int units, const float* prepared_bwd, float* gx, float* gh, float* hprev, int64_t batch,
                          rs_stream_t stream) {
  if (batch == 0) return RS_OK;
  RnnBwdArgs a{};
  const int rc = bwd_args(a, "rs_gru_bwd", saved, T, units, prepared_bwd, batch);
  if (rc != RS_OK) return rc;
  RS_REQUIRE(dseq || dlast, "rs_gru_bwd: null pointer (dseq and dlast)");
  RS_REQUIRE(!dlast || dlast_stride >= units, "rs_gru_bwd: dlast_stride smaller than units");
  RS_REQUIRE(gx && gh && hprev, "rs_gru_bwd: null pointer (gx, gh, hprev)");
  a.dseq = dseq;
  a.dlast = dlast;
  a.dls = dlast_stride;
  a.gx = gx;
  a.gh = gh;
  a.hp = hprev;
  dien_gru_bwd<<<(unsigned)((batch + 15) / 16), DN_MAXG * 64, 0, as_stream(stream)>>>(a);
  return launch_status("rs_gru_bwd");
}

extern "C" int rs_augru_bwd(const float* saved, const float* scores, int64_t scores_stride, const void* len,
                            int len_kind, int weight_norm, const float* dlast, int64_t dlast_stride, int T, int units,
                            int augru_update, const float* prepared_bwd, float* gx, float* hrh, float* ds, float* da,
                            int64_t batch, rs_stream_t stream) {
  if (batch == 0) return RS_OK;
  RnnBwdArgs a{};
  const int rc = bwd_args(a, "rs_augru_bwd", saved, T, units, prepared_bwd, batch);
  if (rc != RS_OK) return rc;
  RS_REQUIRE(scores && len && dlast, "rs_augru_bwd: null pointer (scores, len, dlast)");
  RS_REQUIRE(scores_stride >= T && dlast_stride >= units, "rs_augru_bwd: bad scores_stride / dlast_stride");
  RS_REQUIRE(len_kind == RS_ID_I32 || len_kind == RS_ID_I64, "rs_augru_bwd: len_kind %d (int32 or int64)", len_kind);
  RS_REQUIRE(augru_update == 0 || augru_update == 1, "rs_augru_bwd: augru_update %d (0 reference, 1 paper)",
             augru_update);
  RS_REQUIRE(gx && hrh && ds, "rs_augru_bwd: null pointer (gx, hrh, ds)");
  a.scores = scores;
  a.ssb = scores_stride;
  a.len = len;
  a.len_kind = len_kind;
  a.norm = weight_norm ? 1 : 0;
  a.paper = augru_update;
  a.dlast = dlast;
  a.dls = dlast_stride;
  a.gx = gx;
  a.hp = hrh;
  a.ds = ds;
  a.da = da;
  dien_augru_bwd<<<(unsigned)((batch + 15) / 16), DN_MAXG * 64, 0, as_stream(stream)>>>(a);
  return launch_status("rs_augru_bwd");
}
