// dien.hip — DIEN's interest evolution (model/dien.py:54-70) in one launch:
//   gru1   Keras GRU(D, return_sequences=True), reset_after=True, gates z r h
//          xi = x_t W + bias[0], hr = h U + bias[1]
//          z = sig(xi_z + hr_z), r = sig(xi_r + hr_r), hh = tanh(xi_h + r hr_h)
//          h <- z h + (1 - z) hh                       H1[b, t] = h
//   scores AttentionSequencePoolingLayer(return_score=True) (layer/sequence.py:
//          237-273) over LocalActivationUnit (layer/core.py:94-108):
//          e_t = [q, H1_t, q - H1_t, q H1_t] -> Dense + act, Dense + act,
//          . kernel + bias; positions t >= len masked (-2^32 + 1, softmax over
//          T) or, without weight normalisation, set to 0
//   gru2   AUGRU over AUGRUCell (layer/sequence.py:293-395, layer/activation.py:
//          91-142), no bias, hard_sigmoid gates, a = score[b, t]:
//          z = a hsig(x W_z + h U_z), r = hsig(x W_r + h U_r)
//          hh = tanh(x W_h + (r h) U_h), h <- z h + (1 - z) hh
//          ("paper": h <- (1 - z) h + z hh)            hist[b] = h after T steps
//
// Layout and schedule (gfx950, fp32 v_mfma_f32_16x16x4_f32):
//   * A workgroup owns 16 samples and DN_NW waves.  Every matmul runs in the
//     swapped orientation C^T = W^T x^T of din.hip: the MFMA's A operand is a
//     weight B-fragment in mlp_tower.hpp's packed order (lane l, element j:
//     W[16 g + 4 (l >> 4) + j][16 c + (l & 15)]), its B operand the data (lane
//     l: sample l & 15, the same k), so lane l's accumulator element r is unit
//     16 c + 4 (l >> 4) + r of sample l & 15 — four consecutive units of ONE
//     sample.  A column of the MFMA is a sample: a row's result never depends
//     on its tile mates, on the batch or on the optional outputs.
//   * LDS: seq [T][16][Dp] | hbuf [16][Dp] | rh [16][Dp] | sc [T][16].  seq
//     first holds the tile's keys (staged once by all waves, from the dense
//     keys or gathered through the ids — the only place the two sources
//     differ), then step t of gru1 overwrites x_t with h_t (x_t was consumed
//     one step earlier), so after gru1 it is H1 and gru2 reads its inputs
//     where gru1 left them.  A tile row's 4-float chunks are rotated by the
//     row (chunk q of row s at (q + s) mod Dp/4): the 16 rows of a
//     ds_read_b128 spread over the banks without padding the rows.
//   * Recurrences: wave c < Dp/16 owns units 16 c .. 16 c + 15 of all three
//     gates, its W and U fragments (3 Dp/16 float4 each) in registers for the
//     whole loop and the state of its units in registers; the gate math needs
//     no exchange.  The state tile goes through LDS once per dependent matmul:
//     one barrier per gru1 step, two per gru2 step (r h before U_h).  The
//     input projection of step t + 1 does not depend on the state: it is
//     issued after step t's state store, before the barrier, so its MFMAs run
//     while the other waves arrive.
//   * Scores: wave w takes positions w, w + DN_NW, ...  Layer 1 is regrouped as
//     q (Wq + Wd) + b  (once per wave: the accumulators' C input)
//     + H1_t (Wk - Wd) + (q H1_t) Wp: 2 D MAC rows per position instead of 4 D.
//     Layer 1's accumulators are layer 2's B operand in registers.  The
//     attention weights are read through L1/L2 (<= 100 KB, shared by every
//     workgroup): staged in LDS they would take their size out of T.
//   * One thread per sample then masks / normalises the T scores in t order.
// The recurrences' device functions live in dien_rnn.hpp (shared with the
// training forwards of dien_train.hip).
#include "concat.hpp"
#include "dien_rnn.hpp"
#include "mlp_tower.hpp"

namespace rs {

constexpr int DN_NW = 8;      // waves per workgroup
constexpr int DN_MAXHT = 8;   // 16-unit blocks of an attention layer: width <= 128
constexpr int DN_MAXF = 4;    // behaviour features of the ids form
constexpr int DN_LDS = 160 * 1024;

// ---- packed images
// attention image (depth 2, widths A1 A2; A1p A2p rounded up to 16):
//   [Wkd | Wp | Wqd: A1p/16 tiles x Dp/16 k-groups x 256 each | b1 [A1p] |
//    dice1 (mean, rstd, alpha) [3][A1p] | W2: A2p/16 tiles x A1p/16 k-groups x
//    256 | b2 [A2p] | dice2 [3][A2p] | w3 [A2p] | b3 [4]]
struct AttGeom {
  int A1, A2, A1p, A2p, HT1, HT2;
  int64_t wkd, wp, wqd, b1, d1, w2, b2, d2, w3, b3, size;
};
static bool att_geom(int Dp, int n_layers, const int* hidden, AttGeom& g) {
  if (n_layers != 2 || !hidden) return false;
  if (hidden[0] < 1 || hidden[1] < 1 || hidden[0] > 16 * DN_MAXHT || hidden[1] > 16 * DN_MAXHT) return false;
  g.A1 = hidden[0];
  g.A2 = hidden[1];
  g.A1p = rup(g.A1, 16);
  g.A2p = rup(g.A2, 16);
  g.HT1 = g.A1p / 16;
  g.HT2 = g.A2p / 16;
  int64_t o = 0;
  g.wkd = o; o += (int64_t)g.A1p * Dp;
  g.wp = o; o += (int64_t)g.A1p * Dp;
  g.wqd = o; o += (int64_t)g.A1p * Dp;
  g.b1 = o; o += g.A1p;
  g.d1 = o; o += 3 * g.A1p;
  g.w2 = o; o += (int64_t)g.A2p * g.A1p;
  g.b2 = o; o += g.A2p;
  g.d2 = o; o += 3 * g.A2p;
  g.w3 = o; o += g.A2p;
  g.b3 = o; o += 4;
  g.size = o;
  return true;
}
struct DienGeom {
  GruGeom g1, g2;
  AttGeom at;
  int T, D, Dp, G;
  int64_t o1, o2, oa, size;  // prepared = [gru1 image | gru2 image | attention image]
  size_t lds;
};
static size_t dien_lds(int T, int Dp) { return (size_t)4 * ((size_t)16 * T * Dp + 32 * Dp + (size_t)16 * T); }
static bool dien_act_ok(int act) { return act == RS_ACT_RELU || act == RS_ACT_SIGMOID || act == RS_ACT_DICE; }
// T = 0: the weight image alone (no LDS question)
static bool dien_geom(int T, int D, int n_layers, const int* hidden, DienGeom& g) {
  if (T < 0 || !gru_geom(D, D, g.g1) || !gru_geom(D, D, g.g2)) return false;
  g.T = T;
  g.D = D;
  g.Dp = g.g1.Up;
  g.G = g.g1.G;
  if (!att_geom(g.Dp, n_layers, hidden, g.at)) return false;
  g.o1 = 0;
  g.o2 = g.g1.size;
  g.oa = g.o2 + g.g2.size;
  g.size = g.oa + g.at.size;
  if ((int64_t)T * g.Dp > (int64_t)DN_LDS) return false;  // (keeps dien_lds in range)
  g.lds = dien_lds(T, g.Dp);
  return g.lds <= (size_t)DN_LDS;
}

// out element r of a packed matrix of `ngate` column blocks [K, N] (block b's
// columns at b * N of W, rows ld apart): v = W[ro1 + k] + sgn * W[ro2 + k]
struct PackArgs {
  const float* W;
  int64_t ld;
  int ro1, ro2;
  float sgn;
  int K, N, Kp, Np, ngate;
  float* out;
};
__global__ void dien_pack(PackArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)a.ngate * a.Kp * a.Np) return;
  const int j = (int)(i & 3), lane = (int)((i >> 2) & 63);
  const int64_t blk = i >> 8;
  const int Gk = a.Kp / 16, Gt = a.Np / 16;
  const int g = (int)(blk % Gk), tt = (int)(blk / Gk), gate = tt / Gt, t = tt - gate * Gt;
  const int k = 16 * g + 4 * (lane >> 4) + j, n = 16 * t + (lane & 15);
  float v = 0.f;
  if (k < a.K && n < a.N) {
    const int64_t c = (int64_t)gate * a.N + n;
    v = a.W[(a.ro1 + k) * a.ld + c];
    if (a.sgn != 0.f) v += a.sgn * a.W[(a.ro2 + k) * a.ld + c];
  }
  a.out[i] = v;
}
// rows x [n] -> rows x [np] (zero padded); mode 1: 1 / sqrt(v + 1e-9) (Dice's
// inference normalisation), mode 2: a constant fill `cv` where src is null
__global__ void dien_pack_rows(const float* src, int rows, int n, int np, int mode, float cv, float* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * np) return;
  const int r = i / np, c = i - r * np;
  float v = 0.f;
  if (c < n) {
    v = src ? src[r * n + c] : cv;
    if (mode == 1) v = 1.0f / sqrtf(v + 1e-9f);
  }
  out[i] = v;
}

// ---- device side (the recurrences: dien_rnn.hpp)
__device__ __forceinline__ float dn_act(float x, int act, float mean, float rstd, float alpha) {
  if (act == RS_ACT_RELU) return fmaxf(x, 0.f);
  if (act == RS_ACT_SIGMOID) return sigmoidf_(x);
  const float p = sigmoidf_((x - mean) * rstd);  // Dice at inference (layer/activation.py:32-66)
  return alpha * (1.0f - p) * x + p * x;
}

// one value of a concatenated id source: column j of piece p (kw wide), its id
// at element off of the piece's ids (an out-of-range id: 0, bad = true)
__device__ __forceinline__ float dn_piece_at(const ConcatArgs& a, int p, int j, int kw, int64_t off, bool& bad) {
  int64_t id = 0;
  bool ok;
  switch (a.kind[p]) {
    case RS_ID_I32: ok = cc_id<0>(a.src[p], off, a.vocab[p], id); break;
    case RS_ID_I64: ok = cc_id<1>(a.src[p], off, a.vocab[p], id); break;
    default: ok = cc_id<2>(a.src[p], off, a.vocab[p], id); break;
  }
  bad |= !ok;
  return ok ? a.table[p][id * kw + j] : 0.f;
}
// the piece that holds concatenated column k
__device__ __forceinline__ int dn_piece_of(const ConcatArgs& a, int k) {
  int p = 0;
  for (int i = 1; i < a.np; ++i)
    if (k >= a.col0[i]) p = i;
  return p;
}
// column k of sample b, the ids at b * stride + toff
__device__ __forceinline__ float dn_piece(const ConcatArgs& a, int k, int64_t b, int64_t toff, bool& bad) {
  const int p = dn_piece_of(a, k);
  return dn_piece_at(a, p, k - a.col0[p], a.col0[p + 1] - a.col0[p], b * a.src_stride[p] + toff, bad);
}

__device__ __forceinline__ int64_t dn_len(const void* len, int kind, int64_t b) {
  return kind == RS_ID_I64 ? static_cast<const int64_t*>(len)[b] : (int64_t) static_cast<const int32_t*>(len)[b];
}

struct DienArgs {
  int ids;  // 0: dense keys / q, 1: the id sources
  const float* keys;
  int64_t ksb, kst;
  const float* q;
  int64_t qs;
  ConcatArgs hist, cand;  // ids form: hist ids at b * stride + t, cand ids at b * stride
  const void* len;
  int len_kind;
  const float* prep;
  int64_t o1, o2, oa;
  GruGeom g1;
  AttGeom at;
  int T, D, Dp, G, act, norm, paper;
  float* H1;      // [B, T, D] or null
  float* scores;  // [B, T] or null
  float* out;     // [B, D], rows os apart
  int64_t os;
  int64_t M;
  int* err;
};

__global__ __launch_bounds__(DN_NW * 64) void dien_evolution(DienArgs a) {
  extern __shared__ float smem[];
  const int T = a.T, D = a.D, Dp = a.Dp, G = a.G, NC = 4 * G;
  float* seq = smem;                       // [T][16][Dp]
  float* hbuf = seq + (size_t)T * 16 * Dp;  // [16][Dp]
  float* rh = hbuf + 16 * Dp;              // [16][Dp]
  float* sc = rh + 16 * Dp;                // [T][16]
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int s = lane & 15, kk = lane >> 4;
  const int64_t m0 = (int64_t)blockIdx.x * 16;
  const int64_t mrow = m0 + s < a.M ? m0 + s : a.M - 1;  // rows past the batch re-read the last row, never stored
  const bool live = m0 + s < a.M;
  bool bad = false;

  // ---- the tile's keys into seq (x_t at tile t); hbuf zeroed for gru2
  // a thread owns element (row, k) of every tile: the feature it belongs to is
  // found once, and the T loads of the element (consecutive ids of one row)
  // are independent of each other
  for (int e = threadIdx.x; e < 16 * Dp; e += DN_NW * 64) {
    const int k = e % Dp, row = e / Dp;
    const int64_t b = m0 + row < a.M ? m0 + row : a.M - 1;
    float* dst = seq + dn_off(row, k >> 2, NC) + (k & 3);
    if (k >= D) {
      for (int t = 0; t < T; ++t) dst[(size_t)t * 16 * Dp] = 0.f;
    } else if (!a.ids) {
      const float* src = a.keys + b * a.ksb + k;
#pragma unroll 4
      for (int t = 0; t < T; ++t) dst[(size_t)t * 16 * Dp] = src[t * a.kst];
    } else {
      const int p = dn_piece_of(a.hist, k), j = k - a.hist.col0[p], kw = a.hist.col0[p + 1] - a.hist.col0[p];
      const int64_t off = b * a.hist.src_stride[p], vocab = a.hist.vocab[p];
      const void* src = a.hist.src[p];
      const float* tab = a.hist.table[p] + j;
      // the id kind chosen once around the loop: its body is then a plain
      // load -> load chain the compiler can keep eight deep
      auto rows = [&](auto KIND) {
#pragma unroll 8
        for (int t = 0; t < T; ++t) {
          int64_t id;
          const bool ok = cc_id<decltype(KIND)::value>(src, off + t, vocab, id);
          bad |= !ok;
          const float v = tab[id * kw];  // (id 0 when out of range: in bounds)
          dst[(size_t)t * 16 * Dp] = ok ? v : 0.f;
        }
      };
      switch (a.hist.kind[p]) {
        case RS_ID_I32: rows(std::integral_constant<int, 0>()); break;
        case RS_ID_I64: rows(std::integral_constant<int, 1>()); break;
        default: rows(std::integral_constant<int, 2>()); break;
      }
    }
  }
  for (int i = threadIdx.x; i < 16 * Dp; i += DN_NW * 64) hbuf[i] = 0.f;
  __syncthreads();

  auto tile = [&](int t) { return seq + (size_t)t * 16 * Dp; };
  int aoff[DN_MAXG];
#pragma unroll
  for (int g = 0; g < DN_MAXG; ++g) aoff[g] = g < G ? dn_off(s, 4 * g + kk, NC) : 0;
  auto xseq = [&](int t, int g) { return *reinterpret_cast<const floatx4*>(tile(t) + aoff[g]); };

  // ---- gru1: seq becomes H1
  {
    const float* p = a.prep + a.o1;
    const GruImg im{p + a.g1.w, p + a.g1.u, p + a.g1.b, G, G, Dp};
    dn_gru(
        im, T, xseq, [&](int t) { return tile(t - 1); }, tile,
        [&](int t, const floatx4& h) {
          if (a.H1 && live) {
            float* o = a.H1 + ((m0 + s) * T + t) * D;
            const int u = 16 * w + 4 * kk;
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (u + r < D) o[u + r] = h[r];
          }
        },
        DnNoSave());
  }

  // ---- scores: position t of the 16 samples on wave t mod DN_NW
  {
    const AttGeom& g = a.at;
    const float* p = a.prep + a.oa;
    const int HT1 = g.HT1, HT2 = g.HT2, act = a.act;
    floatx4 qf[DN_MAXG];
#pragma unroll
    for (int gi = 0; gi < DN_MAXG; ++gi) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = 16 * gi + 4 * kk + j;
        float v = 0.f;
        if (gi < G && k < D) v = a.ids ? dn_piece(a.cand, k, mrow, 0, bad) : a.q[mrow * a.qs + k];
        qf[gi][j] = v;
      }
    }
    const floatx4* Wkd = reinterpret_cast<const floatx4*>(p + g.wkd);
    const floatx4* Wp = reinterpret_cast<const floatx4*>(p + g.wp);
    const floatx4* Wqd = reinterpret_cast<const floatx4*>(p + g.wqd);
    const floatx4* W2 = reinterpret_cast<const floatx4*>(p + g.w2);
    auto vec4 = [&](int64_t off, int ht) { return reinterpret_cast<const floatx4*>(p + off + 16 * ht)[kk]; };
    // q (Wq + Wd) + b1: the same for every position
    floatx4 c1[DN_MAXHT];
#pragma unroll
    for (int ht = 0; ht < DN_MAXHT; ++ht) {
      c1[ht] = floatx4{0.f, 0.f, 0.f, 0.f};
      if (ht < HT1 && w < T) {
        floatx4 acc = vec4(g.b1, ht);
#pragma unroll
        for (int gi = 0; gi < DN_MAXG; ++gi) {
          if (gi < G) {
            const floatx4 wv = (Wqd + (ht * G + gi) * 64)[lane];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = mfma16x16x4(wv[j], qf[gi][j], acc);
          }
        }
        c1[ht] = acc;
      }
    }
    const float b3 = p[g.b3];
    for (int t = w; t < T; t += DN_NW) {
      // the weight fragments are re-read (L1 / L2) per position and their
      // addresses formed at the load (ln: the lane, opaque per iteration):
      // hoisted out of the loop, the up to 320 address pairs per lane spilled
      // 158 VGPRs
      int ln = lane;
      asm volatile("" : "+v"(ln)::"memory");
      floatx4 hf[DN_MAXG], pf[DN_MAXG];
#pragma unroll
      for (int gi = 0; gi < DN_MAXG; ++gi) {
        hf[gi] = gi < G ? xseq(t, gi) : floatx4{0.f, 0.f, 0.f, 0.f};
        pf[gi] = hf[gi] * qf[gi];
      }
      floatx4 y1[DN_MAXHT];
#pragma unroll
      for (int ht = 0; ht < DN_MAXHT; ++ht) {
        y1[ht] = floatx4{0.f, 0.f, 0.f, 0.f};
        if (ht < HT1) {
          floatx4 ak = c1[ht], ap = {0.f, 0.f, 0.f, 0.f};  // two chains
#pragma unroll
          for (int gi = 0; gi < DN_MAXG; ++gi) {
            if (gi < G) {
              const floatx4 wk = (Wkd + (ht * G + gi) * 64)[ln], wp = (Wp + (ht * G + gi) * 64)[ln];
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                ak = mfma16x16x4(wk[j], hf[gi][j], ak);
                ap = mfma16x16x4(wp[j], pf[gi][j], ap);
              }
            }
          }
          floatx4 mean = {0.f, 0.f, 0.f, 0.f}, rstd = mean, alpha = mean;
          if (act == RS_ACT_DICE) {
            mean = vec4(g.d1, ht);
            rstd = vec4(g.d1 + g.A1p, ht);
            alpha = vec4(g.d1 + 2 * g.A1p, ht);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) y1[ht][r] = dn_act(ak[r] + ap[r], act, mean[r], rstd[r], alpha[r]);
        }
      }
      float part = 0.f;
#pragma unroll
      for (int h2 = 0; h2 < DN_MAXHT; ++h2) {
        if (h2 < HT2) {
          floatx4 acc = vec4(g.b2, h2);
#pragma unroll
          for (int ht = 0; ht < DN_MAXHT; ++ht) {
            if (ht < HT1) {
              const floatx4 wv = (W2 + (h2 * HT1 + ht) * 64)[ln];
#pragma unroll
              for (int r = 0; r < 4; ++r) acc = mfma16x16x4(wv[r], y1[ht][r], acc);
            }
          }
          floatx4 mean = {0.f, 0.f, 0.f, 0.f}, rstd = mean, alpha = mean;
          if (act == RS_ACT_DICE) {
            mean = vec4(g.d2, h2);
            rstd = vec4(g.d2 + g.A2p, h2);
            alpha = vec4(g.d2 + 2 * g.A2p, h2);
          }
          const floatx4 w3 = vec4(g.w3, h2);
#pragma unroll
          for (int r = 0; r < 4; ++r) part = fmaf(dn_act(acc[r], act, mean[r], rstd[r], alpha[r]), w3[r], part);
        }
      }
      part += __shfl_xor(part, 16);
      part += __shfl_xor(part, 32);
      if (kk == 0) sc[t * 16 + s] = part + b3;
    }
  }
  if (__any(bad) && lane == 0) flag_error(a.err);
  __syncthreads();

  // ---- mask / normalise: one thread per sample, t ascending
  if (threadIdx.x < 16) {
    const int64_t L = dn_len(a.len, a.len_kind, mrow);
    float* so = a.scores && live ? a.scores + (m0 + s) * T : nullptr;
    if (a.norm) {
      float mx = -INFINITY;
      for (int t = 0; t < T; ++t) {
        const float v = t < L ? sc[t * 16 + s] : -4294967296.0f;  // -2^32 + 1 in fp32
        sc[t * 16 + s] = v;
        mx = fmaxf(mx, v);
      }
      float sum = 0.f;
      for (int t = 0; t < T; ++t) {
        const float e = expf(sc[t * 16 + s] - mx);
        sc[t * 16 + s] = e;
        sum += e;
      }
      for (int t = 0; t < T; ++t) {
        const float v = sc[t * 16 + s] / sum;
        sc[t * 16 + s] = v;
        if (so) so[t] = v;
      }
    } else {
      for (int t = 0; t < T; ++t) {
        const float v = t < L ? sc[t * 16 + s] : 0.f;
        sc[t * 16 + s] = v;
        if (so) so[t] = v;
      }
    }
  }
  __syncthreads();

  // ---- gru2 over H1 with the scores
  {
    const float* p = a.prep + a.o2;
    const GruImg im{p + a.g1.w, p + a.g1.u, p + a.g1.b, G, G, Dp};
    floatx4 h;
    dn_augru(
        im, T, a.paper, xseq, [&](int t) { return sc[t * 16 + s]; }, hbuf, rh, h, DnNoSave());
    if (w < G && live) {
      float* o = a.out + (m0 + s) * a.os;
      const int u = 16 * w + 4 * kk;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (u + r < D) o[u + r] = h[r];
    }
  }
}

static void pack_matrix(const float* W, int64_t ld, int ro1, int ro2, float sgn, int K, int N, int Kp, int Np, int ngate,
                        float* out, hipStream_t st) {
  PackArgs p{W, ld, ro1, ro2, sgn, K, N, Kp, Np, ngate, out};
  const int64_t n = (int64_t)ngate * Kp * Np;
  dien_pack<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(p);
}
static void pack_rows(const float* src, int rows, int n, int np, int mode, float cv, float* out, hipStream_t st) {
  dien_pack_rows<<<(unsigned)((rows * np + 255) / 256), 256, 0, st>>>(src, rows, n, np, mode, cv, out);
}
static void gru_pack(const GruGeom& g, const float* kernel, const float* recurrent, const float* bias, float* out,
                     hipStream_t st) {
  pack_matrix(kernel, 3ll * g.U, 0, 0, 0.f, g.din, g.U, g.Kp, g.Up, 3, out + g.w, st);
  pack_matrix(recurrent, 3ll * g.U, 0, 0, 0.f, g.U, g.U, g.Up, g.Up, 3, out + g.u, st);
  pack_rows(bias, 6, g.U, g.Up, bias ? 0 : 2, 0.f, out + g.b, st);  // [2][3 U] read as 6 rows of U
}

}  // namespace rs

using namespace rs;

#define DIEN_SHAPE_MSG \
  "need 1 <= D <= %d, exactly 2 attention layers 1..%d wide, and 4 * (16 T Dp + 32 Dp + 16 T) <= %d bytes of LDS"
#define DIEN_SHAPE_ARGS 16 * DN_MAXG, 16 * DN_MAXHT, DN_LDS

extern "C" int rs_dien_evolution_ok(int T, int D, int n_att_layers, const int* att_hidden, int att_act) {
  DienGeom g;
  return T >= 1 && dien_act_ok(att_act) && dien_geom(T, D, n_att_layers, att_hidden, g) ? 1 : 0;
}

extern "C" int64_t rs_dien_prepared_size(int D, int n_att_layers, const int* att_hidden) {
  DienGeom g;
  if (!dien_geom(0, D, n_att_layers, att_hidden, g)) {
    set_error("rs_dien_prepared_size: " DIEN_SHAPE_MSG, DIEN_SHAPE_ARGS);
    return -1;
  }
  return g.size;
}

extern "C" int64_t rs_gru_prepared_size(int din, int units) {
  GruGeom g;
  if (!gru_geom(din, units, g)) {
    set_error("rs_gru_prepared_size: need 1 <= din, units <= %d", 16 * DN_MAXG);
    return -1;
  }
  return g.size;
}

extern "C" int rs_gru_prepare(int din, int units, const float* kernel, const float* recurrent, const float* bias,
                              float* prepared, rs_stream_t stream) {
  GruGeom g;
  RS_REQUIRE(gru_geom(din, units, g), "rs_gru_prepare: need 1 <= din, units <= %d", 16 * DN_MAXG);
  RS_REQUIRE(kernel && recurrent && prepared, "rs_gru_prepare: null pointer (kernel, recurrent, prepared)");
  gru_pack(g, kernel, recurrent, bias, prepared, as_stream(stream));
  return launch_status("rs_gru_prepare");
}

extern "C" int rs_dien_prepare(int D, const float* gru1_kernel, const float* gru1_recurrent, const float* gru1_bias,
                               const float* gru2_kernel, const float* gru2_recurrent, int n_att_layers,
                               const int* att_hidden, int att_act, const float* const* att_W,
                               const float* const* att_b, const float* const* dice_mean,
                               const float* const* dice_var, const float* const* dice_alpha, const float* att_out_w,
                               const float* att_out_b, float* prepared, rs_stream_t stream) {
  DienGeom g;
  RS_REQUIRE(dien_geom(0, D, n_att_layers, att_hidden, g), "rs_dien_prepare: " DIEN_SHAPE_MSG, DIEN_SHAPE_ARGS);
  RS_REQUIRE(dien_act_ok(att_act), "rs_dien_prepare: att_act %d (relu 1, sigmoid 3 or dice 4)", att_act);
  RS_REQUIRE(gru1_kernel && gru1_recurrent && gru1_bias && gru2_kernel && gru2_recurrent && att_W && att_b &&
                 att_out_w && att_out_b && prepared,
             "rs_dien_prepare: null pointer");
  const bool dice = att_act == RS_ACT_DICE;
  for (int l = 0; l < 2; ++l) {
    RS_REQUIRE(att_W[l] && att_b[l], "rs_dien_prepare: attention layer %d has no kernel / bias", l);
    RS_REQUIRE(!dice || (dice_mean && dice_var && dice_alpha && dice_mean[l] && dice_var[l] && dice_alpha[l]),
               "rs_dien_prepare: dice needs mean, variance and alpha of attention layer %d", l);
  }
  hipStream_t st = as_stream(stream);
  gru_pack(g.g1, gru1_kernel, gru1_recurrent, gru1_bias, prepared + g.o1, st);
  gru_pack(g.g2, gru2_kernel, gru2_recurrent, nullptr, prepared + g.o2, st);
  const AttGeom& t = g.at;
  float* o = prepared + g.oa;
  // W1 [4 D, A1] = [Wq; Wk; Wd; Wp]
  pack_matrix(att_W[0], t.A1, D, 2 * D, -1.f, D, t.A1, g.Dp, t.A1p, 1, o + t.wkd, st);
  pack_matrix(att_W[0], t.A1, 3 * D, 0, 0.f, D, t.A1, g.Dp, t.A1p, 1, o + t.wp, st);
  pack_matrix(att_W[0], t.A1, 0, 2 * D, 1.f, D, t.A1, g.Dp, t.A1p, 1, o + t.wqd, st);
  pack_rows(att_b[0], 1, t.A1, t.A1p, 0, 0.f, o + t.b1, st);
  pack_matrix(att_W[1], t.A2, 0, 0, 0.f, t.A1, t.A2, t.A1p, t.A2p, 1, o + t.w2, st);
  pack_rows(att_b[1], 1, t.A2, t.A2p, 0, 0.f, o + t.b2, st);
  const int Ap[2] = {t.A1p, t.A2p}, A[2] = {t.A1, t.A2};
  const int64_t doff[2] = {t.d1, t.d2};
  for (int l = 0; l < 2; ++l) {
    pack_rows(dice ? dice_mean[l] : nullptr, 1, A[l], Ap[l], dice ? 0 : 2, 0.f, o + doff[l], st);
    pack_rows(dice ? dice_var[l] : nullptr, 1, A[l], Ap[l], dice ? 1 : 2, 0.f, o + doff[l] + Ap[l], st);
    pack_rows(dice ? dice_alpha[l] : nullptr, 1, A[l], Ap[l], dice ? 0 : 2, 0.f, o + doff[l] + 2 * Ap[l], st);
  }
  pack_rows(att_out_w, 1, t.A2, t.A2p, 0, 0.f, o + t.w3, st);
  pack_rows(att_out_b, 1, 1, 4, 0, 0.f, o + t.b3, st);
  return launch_status("rs_dien_prepare");
}

static int dien_launch(DienArgs& a, const char* what, int T, int D, int n_att_layers, const int* att_hidden,
                       int att_act, int weight_norm, int augru_update, const void* len, int len_kind,
                       const float* prepared, float* H1, float* scores, float* hist, int64_t hist_stride,
                       int64_t batch, int* err_flag, rs_stream_t stream) {
  DienGeom g;
  RS_REQUIRE(T >= 1 && dien_geom(T, D, n_att_layers, att_hidden, g), "%s: " DIEN_SHAPE_MSG, what, DIEN_SHAPE_ARGS);
  RS_REQUIRE(dien_act_ok(att_act), "%s: att_act %d (relu 1, sigmoid 3 or dice 4)", what, att_act);
  RS_REQUIRE(augru_update == 0 || augru_update == 1, "%s: augru_update %d (0 reference, 1 paper)", what, augru_update);
  RS_REQUIRE(len && prepared && hist, "%s: null pointer (len, prepared, hist)", what);
  RS_REQUIRE(len_kind == RS_ID_I32 || len_kind == RS_ID_I64, "%s: len_kind %d (int32 or int64)", what, len_kind);
  RS_REQUIRE(batch > 0 && hist_stride >= D, "%s: bad batch / hist_stride < D", what);
  const int64_t grid = (batch + 15) / 16;
  RS_REQUIRE(grid < (1ll << 31) && batch * T < (1ll << 40), "%s: batch too large", what);
  a.len = len;
  a.len_kind = len_kind;
  a.prep = prepared;
  a.o1 = g.o1;
  a.o2 = g.o2;
  a.oa = g.oa;
  a.g1 = g.g1;
  a.at = g.at;
  a.T = T;
  a.D = D;
  a.Dp = g.Dp;
  a.G = g.G;
  a.act = att_act;
  a.norm = weight_norm ? 1 : 0;
  a.paper = augru_update;
  a.H1 = H1;
  a.scores = scores;
  a.out = hist;
  a.os = hist_stride;
  a.M = batch;
  a.err = err_flag;
  launch_lds<dien_evolution>((unsigned)grid, DN_NW * 64, g.lds, as_stream(stream), a);
  return launch_status(what);
}

extern "C" int rs_dien_evolution_fwd(const float* keys, int64_t keys_bstride, int64_t keys_tstride, const float* q,
                                     int64_t q_stride, const void* len, int len_kind, int T, int D,
                                     int n_att_layers, const int* att_hidden, int att_act, int weight_norm,
                                     int augru_update, const float* prepared, float* H1, float* scores, float* hist,
                                     int64_t hist_stride, int64_t batch, rs_stream_t stream) {
  if (batch == 0) return RS_OK;
  RS_REQUIRE(keys && q, "rs_dien_evolution_fwd: null pointer (keys, q)");
  RS_REQUIRE(D >= 1 && keys_tstride >= D && T >= 1 && keys_bstride >= (int64_t)(T - 1) * keys_tstride + D &&
                 q_stride >= D,
             "rs_dien_evolution_fwd: bad strides");
  DienArgs a{};
  a.ids = 0;
  a.keys = keys;
  a.ksb = keys_bstride;
  a.kst = keys_tstride;
  a.q = q;
  a.qs = q_stride;
  return dien_launch(a, "rs_dien_evolution_fwd", T, D, n_att_layers, att_hidden, att_act, weight_norm, augru_update,
                     len, len_kind, prepared, H1, scores, hist, hist_stride, batch, nullptr, stream);
}

extern "C" int rs_dien_evolution_ids_fwd(int n_feat, const int* widths, const int* kinds,
                                         const void* const* hist_ids, const int64_t* hist_strides,
                                         const void* const* cand_ids, const int64_t* cand_strides,
                                         const float* const* tables, const int64_t* vocabs, const void* len,
                                         int len_kind, int T, int D, int n_att_layers, const int* att_hidden,
                                         int att_act, int weight_norm, int augru_update, const float* prepared,
                                         float* H1, float* scores, float* hist, int64_t hist_stride, int64_t batch,
                                         int* err_flag, rs_stream_t stream) {
  if (batch == 0) return RS_OK;
  const char* what = "rs_dien_evolution_ids_fwd";
  RS_REQUIRE(n_feat >= 1 && n_feat <= DN_MAXF, "%s: 1..%d behaviour features", what, DN_MAXF);
  RS_REQUIRE(widths && kinds && hist_ids && hist_strides && cand_ids && cand_strides && tables && vocabs,
             "%s: null pointer", what);
  RS_REQUIRE(T >= 1 && D >= 1, "%s: T, D >= 1", what);
  int cols[DN_MAXF], sum = 0;
  for (int f = 0; f < n_feat; ++f) {
    RS_REQUIRE(kinds[f] >= RS_ID_I32 && kinds[f] <= RS_ID_F32, "%s: feature %d: bad id kind", what, f);
    RS_REQUIRE(hist_strides[f] >= T, "%s: feature %d: hist stride smaller than T", what, f);
    cols[f] = sum;
    sum += widths[f] > 0 ? widths[f] : 0;
  }
  RS_REQUIRE(sum == D, "%s: the widths add up to %d, D is %d", what, sum, D);
  DienArgs a{};
  a.ids = 1;
  int rc = concat_fill(n_feat, widths, cols, kinds, hist_ids, hist_strides, tables, vocabs, D, what, a.hist);
  if (rc != RS_OK) return rc;
  rc = concat_fill(n_feat, widths, cols, kinds, cand_ids, cand_strides, tables, vocabs, D, what, a.cand);
  if (rc != RS_OK) return rc;
  return dien_launch(a, what, T, D, n_att_layers, att_hidden, att_act, weight_norm, augru_update, len, len_kind,
                     prepared, H1, scores, hist, hist_stride, batch, err_flag, stream);
}

extern "C" int rs_gru_fwd(const float* x, int64_t x_bstride, int64_t x_tstride, int T, int din, int units,
                          const float* prepared, float* seq, float* last, int64_t last_stride, int64_t batch,
                          rs_stream_t stream) {
  if (batch == 0) return RS_OK;
  RnnArgs a{};
  const int rc = rnn_args(a, "rs_gru_fwd", x, x_bstride, x_tstride, T, din, units, prepared, batch);
  if (rc != RS_OK) return rc;
  RS_REQUIRE(seq || last, "rs_gru_fwd: null pointer (seq and last)");
  RS_REQUIRE(!last || last_stride >= units, "rs_gru_fwd: last_stride smaller than units");
  a.seq = seq;
  a.last = last;
  a.ls = last_stride;
  dien_rnn<false, false><<<(unsigned)((batch + 15) / 16), DN_MAXG * 64, 0, as_stream(stream)>>>(a);
  return launch_status("rs_gru_fwd");
}

extern "C" int rs_augru_fwd(const float* x, int64_t x_bstride, int64_t x_tstride, const float* scores,
                            int64_t scores_stride, int T, int din, int units, int augru_update,
                            const float* prepared, float* last, int64_t last_stride, int64_t batch,
                            rs_stream_t stream) {
  if (batch == 0) return RS_OK;
  RnnArgs a{};
  const int rc = rnn_args(a, "rs_augru_fwd", x, x_bstride, x_tstride, T, din, units, prepared, batch);
  if (rc != RS_OK) return rc;
  RS_REQUIRE(scores && last, "rs_augru_fwd: null pointer (scores, last)");
  RS_REQUIRE(scores_stride >= T && last_stride >= units, "rs_augru_fwd: bad scores_stride / last_stride");
  RS_REQUIRE(augru_update == 0 || augru_update == 1, "rs_augru_fwd: augru_update %d (0 reference, 1 paper)",
             augru_update);
  a.scores = scores;
  a.ssb = scores_stride;
  a.paper = augru_update;
  a.last = last;
  a.ls = last_stride;
  dien_rnn<true, false><<<(unsigned)((batch + 15) / 16), DN_MAXG * 64, 0, as_stream(stream)>>>(a);
  return launch_status("rs_augru_fwd");
}
