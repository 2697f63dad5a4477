// dien_rnn.hpp — the two recurrences of DIEN as device functions, shared by
// dien.hip (the one-launch interest evolution and the stand-alone forwards)
// and dien_train.hip (the training forwards, which run the SAME functions and
// also store what the backward reads).  Layout and schedule: dien.hip's header.
#pragma once
#include "mlp_tower.hpp"

namespace rs {

constexpr int DN_MAXG = 4;  // 16-unit blocks of the state: D <= 64

// gru image (din inputs, U units; Kp = roundup(din, 16), Up = roundup(U, 16)):
//   [W: 3 gates x Up/16 tiles x Kp/16 k-groups x 64 lanes x 4 | U: the same
//    with Up/16 k-groups | bias: [2][3][Up]]
struct GruGeom {
  int din, U, Kp, Up, Gi, G;
  int64_t w, u, b, size;
};
static bool gru_geom(int din, int U, GruGeom& g) {
  if (din < 1 || U < 1 || din > 16 * DN_MAXG || U > 16 * DN_MAXG) return false;
  g.din = din;
  g.U = U;
  g.Kp = rup(din, 16);
  g.Up = rup(U, 16);
  g.Gi = g.Kp / 16;
  g.G = g.Up / 16;
  g.w = 0;
  g.u = g.w + 3ll * g.Up * g.Kp;
  g.b = g.u + 3ll * g.Up * g.Up;
  g.size = g.b + 6ll * g.Up;
  return true;
}

__device__ __forceinline__ float dn_hsig(float x) { return fminf(fmaxf(0.2f * x + 0.5f, 0.f), 1.f); }

// float offset of chunk q (4 floats) of row s in a rotated [16][Dp] tile
__device__ __forceinline__ int dn_off(int s, int q, int NC) { return s * (4 * NC) + 4 * ((q + s) % NC); }

// this wave's fragments of a gate matrix (tile c of Gt, Gk k-groups)
__device__ __forceinline__ void dn_load_w(const float* pack, int c, int Gt, int Gk, floatx4 (&Wr)[3][DN_MAXG]) {
  const int lane = threadIdx.x & 63;
  const floatx4* p = reinterpret_cast<const floatx4*>(pack) + lane;
#pragma unroll
  for (int gate = 0; gate < 3; ++gate)
#pragma unroll
    for (int g = 0; g < DN_MAXG; ++g)
      Wr[gate][g] = g < Gk ? p[(int64_t)((gate * Gt + c) * Gk + g) * 64] : floatx4{0.f, 0.f, 0.f, 0.f};
}
__device__ __forceinline__ floatx4 dn_bias(const float* bias, int row, int gate, int Up, int c) {
  const int lane = threadIdx.x & 63;
  return *reinterpret_cast<const floatx4*>(bias + (row * 3 + gate) * Up + 16 * c + 4 * (lane >> 4));
}
// acc[gate] += W_gate^T x^T over Gk k-groups, gates gate0 .. gate1 - 1; xf(g): the data fragment
template <class XF>
__device__ __forceinline__ void dn_mac(const floatx4 (&Wr)[3][DN_MAXG], int Gk, int gate0, int gate1, XF xf,
                                       floatx4 (&acc)[3]) {
#pragma unroll
  for (int g = 0; g < DN_MAXG; ++g) {
    if (g < Gk) {
      const floatx4 x = xf(g);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int gate = 0; gate < 3; ++gate)
          if (gate >= gate0 && gate < gate1) acc[gate] = mfma16x16x4(Wr[gate][g][j], x[j], acc[gate]);
    }
  }
}

struct GruImg {
  const float *W, *U, *bias;
  int Gi, G, Up;
};

// what the inference launches pass as `save`
struct DnNoSave {
  __device__ __forceinline__ void operator()(int, const floatx4&, const floatx4&, const floatx4&, const floatx4&,
                                             const floatx4&) const {}
  __device__ __forceinline__ void operator()(int, const floatx4&, const floatx4&, const floatx4&,
                                             const floatx4&) const {}
};

// gru1 on the 16-sample tile.  xf(t, g): fragment g of x_t; hprev(t) / hnext(t):
// the LDS tiles the state before / after step t is read from / written to
// (rotated [16][Up]); emit(t, h): lane's four units of h_t; save(t, z, r, hh,
// hr_h, h_prev): the step's gates of the same four units (training).  All
// waves call it (the barriers); waves >= G only take the barriers.
template <class XF, class HP, class HN, class Emit, class Save>
__device__ __forceinline__ void dn_gru(const GruImg& im, int T, XF xf, HP hprev, HN hnext, Emit emit, Save save) {
  const int lane = threadIdx.x & 63;
  const int c = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int s = lane & 15, kk = lane >> 4, NC = 4 * im.G;
  const bool mine = c < im.G;
  floatx4 Wr[3][DN_MAXG], Ur[3][DN_MAXG], bi[3], br[3], xi[3];
  int aoff[DN_MAXG];
  floatx4 h = {0.f, 0.f, 0.f, 0.f};
  int hoff = 0;
  if (mine) {
    dn_load_w(im.W, c, im.G, im.Gi, Wr);
    dn_load_w(im.U, c, im.G, im.G, Ur);
#pragma unroll
    for (int gate = 0; gate < 3; ++gate) {
      bi[gate] = dn_bias(im.bias, 0, gate, im.Up, c);
      br[gate] = dn_bias(im.bias, 1, gate, im.Up, c);
      xi[gate] = bi[gate];
    }
#pragma unroll
    for (int g = 0; g < DN_MAXG; ++g) aoff[g] = dn_off(s, 4 * g + kk, NC);
    hoff = dn_off(s, 4 * c + kk, NC);
    dn_mac(Wr, im.Gi, 0, 3, [&](int g) { return xf(0, g); }, xi);
  }
  __syncthreads();  // every wave has read x_0 (step 0 may overwrite it with h_0)
  for (int t = 0; t < T; ++t) {
    if (mine) {
      floatx4 hr[3] = {br[0], br[1], br[2]};
      if (t > 0) {
        const float* hp = hprev(t);
        dn_mac(Ur, im.G, 0, 3, [&](int g) { return *reinterpret_cast<const floatx4*>(hp + aoff[g]); }, hr);
      }
      const floatx4 h0 = h;
      floatx4 zv, rv, hv;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float z = sigmoidf_(xi[0][r] + hr[0][r]);
        const float rg = sigmoidf_(xi[1][r] + hr[1][r]);
        const float hh = tanhf(xi[2][r] + rg * hr[2][r]);
        h[r] = z * h[r] + (1.0f - z) * hh;
        zv[r] = z;
        rv[r] = rg;
        hv[r] = hh;
      }
      *reinterpret_cast<floatx4*>(hnext(t) + hoff) = h;
      emit(t, h);
      save(t, zv, rv, hv, hr[2], h0);
      if (t + 1 < T) {
#pragma unroll
        for (int gate = 0; gate < 3; ++gate) xi[gate] = bi[gate];
        dn_mac(Wr, im.Gi, 0, 3, [&](int g) { return xf(t + 1, g); }, xi);
      }
    }
    __syncthreads();  // h_t complete
  }
}

// gru2 (AUGRU).  score(t): a of this lane's sample; hbuf / rh: rotated
// [16][Up] LDS tiles (hbuf zeroed by the caller, barrier taken); returns the
// lane's four units of the last state in h.  save(t, u, r, hh, h_prev) with
// u = hsig(a_z), r = hsig(a_r) (training).
template <class XF, class SF, class Save>
__device__ __forceinline__ void dn_augru(const GruImg& im, int T, int paper, XF xf, SF score, float* hbuf, float* rh,
                                         floatx4& h, Save save) {
  const int lane = threadIdx.x & 63;
  const int c = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int s = lane & 15, kk = lane >> 4, NC = 4 * im.G;
  const bool mine = c < im.G;
  floatx4 Wr[3][DN_MAXG], Ur[3][DN_MAXG], xi[3];
  const floatx4 zero = {0.f, 0.f, 0.f, 0.f};
  int aoff[DN_MAXG];
  int hoff = 0;
  h = zero;
  if (mine) {
    dn_load_w(im.W, c, im.G, im.Gi, Wr);
    dn_load_w(im.U, c, im.G, im.G, Ur);
#pragma unroll
    for (int g = 0; g < DN_MAXG; ++g) aoff[g] = dn_off(s, 4 * g + kk, NC);
    hoff = dn_off(s, 4 * c + kk, NC);
    xi[0] = xi[1] = xi[2] = zero;
    dn_mac(Wr, im.Gi, 0, 3, [&](int g) { return xf(0, g); }, xi);
  }
  for (int t = 0; t < T; ++t) {
    float z[4];
    floatx4 uv, rg;
    const floatx4 h0 = h;
    if (mine) {
      const float a = score(t);
      floatx4 acc[3] = {xi[0], xi[1], zero};
      dn_mac(Ur, im.G, 0, 2, [&](int g) { return *reinterpret_cast<const floatx4*>(hbuf + aoff[g]); }, acc);
      floatx4 rv;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        uv[r] = dn_hsig(acc[0][r]);
        rg[r] = dn_hsig(acc[1][r]);
        z[r] = a * uv[r];
        rv[r] = rg[r] * h[r];
      }
      *reinterpret_cast<floatx4*>(rh + hoff) = rv;
    }
    __syncthreads();  // r h complete
    if (mine) {
      floatx4 acc[3] = {zero, zero, xi[2]};
      dn_mac(Ur, im.G, 2, 3, [&](int g) { return *reinterpret_cast<const floatx4*>(rh + aoff[g]); }, acc);
      floatx4 hv;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float hh = tanhf(acc[2][r]);
        hv[r] = hh;
        h[r] = paper ? (1.0f - z[r]) * h[r] + z[r] * hh : z[r] * h[r] + (1.0f - z[r]) * hh;
      }
      *reinterpret_cast<floatx4*>(hbuf + hoff) = h;
      save(t, uv, rg, hv, h0);
      if (t + 1 < T) {
        xi[0] = xi[1] = xi[2] = zero;
        dn_mac(Wr, im.Gi, 0, 3, [&](int g) { return xf(t + 1, g); }, xi);
      }
    }
    __syncthreads();  // h_t complete
  }
}

// a [16][width] tile of a dense [B, T, width] input at step t, as a fragment
__device__ __forceinline__ floatx4 dn_xglobal(const float* x, int64_t b, int64_t sb, int64_t st, int t, int width,
                                              int g) {
  const int lane = threadIdx.x & 63;
  const int k = 16 * g + 4 * (lane >> 4);
  const float* p = x + b * sb + t * st;
  floatx4 v;
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = k + j < width ? p[k + j] : 0.f;
  return v;
}

// ---- the recurrences alone (the GRU / AUGRU layers, the unfused path): x
// [B, T, din] read from global memory step by step, the state through LDS
constexpr int DN_GRU_PLANES = 5;    // saved[b][t]: z, r, hh, hr_h, h_prev, [Up] each
constexpr int DN_AUGRU_PLANES = 4;  // saved[b][t]: u, r, hh, h_prev
struct RnnArgs {
  const float* x;
  int64_t xsb, xst;
  const float* scores;  // AUGRU: [B, T], rows ssb apart
  int64_t ssb;
  const float* prep;
  GruGeom g;
  int T, paper;
  float* seq;   // GRU: [B, T, U]
  float* last;  // [B, U], rows ls apart (AUGRU; optional for GRU)
  int64_t ls;
  int64_t M;
  float* saved;  // SAVE: [B, T, planes, Up]
};

template <bool AUGRU, bool SAVE>
__global__ __launch_bounds__(DN_MAXG * 64) void dien_rnn(RnnArgs a) {
  __shared__ float hb[2][16 * 16 * DN_MAXG];
  const GruGeom& g = a.g;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int s = lane & 15, kk = lane >> 4;
  const int64_t m0 = (int64_t)blockIdx.x * 16;
  const int64_t mrow = m0 + s < a.M ? m0 + s : a.M - 1;
  const bool live = m0 + s < a.M;
  const GruImg im{a.prep + g.w, a.prep + g.u, a.prep + g.b, g.Gi, g.G, g.Up};
  auto xf = [&](int t, int gi) { return dn_xglobal(a.x, mrow, a.xsb, a.xst, t, g.din, gi); };
  const int u = 16 * w + 4 * kk;
  // plane p of step t, this lane's four units (padded units included: Up wide)
  auto plane = [&](int t, int planes, int p) {
    return reinterpret_cast<floatx4*>(a.saved + (((m0 + s) * a.T + t) * planes + p) * g.Up + u);
  };
  if constexpr (AUGRU) {
    for (int i = threadIdx.x; i < 16 * g.Up; i += DN_MAXG * 64) hb[0][i] = 0.f;
    __syncthreads();
    floatx4 h;
    auto score = [&](int t) { return a.scores[mrow * a.ssb + t]; };
    if constexpr (SAVE) {
      dn_augru(im, a.T, a.paper, xf, score, hb[0], hb[1], h,
               [&](int t, const floatx4& uv, const floatx4& rv, const floatx4& hv, const floatx4& h0) {
                 if (!live) return;
                 *plane(t, DN_AUGRU_PLANES, 0) = uv;
                 *plane(t, DN_AUGRU_PLANES, 1) = rv;
                 *plane(t, DN_AUGRU_PLANES, 2) = hv;
                 *plane(t, DN_AUGRU_PLANES, 3) = h0;
               });
    } else {
      dn_augru(im, a.T, a.paper, xf, score, hb[0], hb[1], h, DnNoSave());
    }
    if (w < g.G && live) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (u + r < g.U) a.last[(m0 + s) * a.ls + u + r] = h[r];
    }
  } else {
    auto hp = [&](int t) { return hb[(t + 1) & 1]; };
    auto hn = [&](int t) { return hb[t & 1]; };
    auto emit = [&](int t, const floatx4& h) {
      if (!live) return;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (u + r < g.U) {
          if (a.seq) a.seq[((m0 + s) * a.T + t) * g.U + u + r] = h[r];
          if (a.last && t == a.T - 1) a.last[(m0 + s) * a.ls + u + r] = h[r];
        }
      }
    };
    if constexpr (SAVE) {
      dn_gru(im, a.T, xf, hp, hn, emit,
             [&](int t, const floatx4& zv, const floatx4& rv, const floatx4& hv, const floatx4& hrh,
                 const floatx4& h0) {
               if (!live) return;
               *plane(t, DN_GRU_PLANES, 0) = zv;
               *plane(t, DN_GRU_PLANES, 1) = rv;
               *plane(t, DN_GRU_PLANES, 2) = hv;
               *plane(t, DN_GRU_PLANES, 3) = hrh;
               *plane(t, DN_GRU_PLANES, 4) = h0;
             });
    } else {
      dn_gru(im, a.T, xf, hp, hn, emit, DnNoSave());
    }
  }
}

static int rnn_args(RnnArgs& a, const char* what, const float* x, int64_t x_bstride, int64_t x_tstride, int T, int din,
                    int units, const float* prepared, int64_t batch) {
  RS_REQUIRE(gru_geom(din, units, a.g), "%s: need 1 <= din, units <= %d", what, 16 * DN_MAXG);
  RS_REQUIRE(x && prepared, "%s: null pointer (x, prepared)", what);
  RS_REQUIRE(T >= 1 && batch > 0 && x_tstride >= din && x_bstride >= (int64_t)(T - 1) * x_tstride + din,
             "%s: bad T / batch / strides", what);
  RS_REQUIRE((batch + 15) / 16 < (1ll << 31), "%s: batch too large", what);
  a.x = x;
  a.xsb = x_bstride;
  a.xst = x_tstride;
  a.prep = prepared;
  a.T = T;
  a.M = batch;
  return RS_OK;
}

}  // namespace rs
