// deepfm.hip — fused DeepFM forward (rs_deepfm_fwd, rs_deepfm_fwd_hm): gather
// + FM + DNN tower + head in one launch.  deepfm_fused / deepfm_fused_ka run
// embed_fm_body (embed_fm_body.hpp) with the tower of mlp_tower.hpp behind it;
// deepfm_ws and deepfm_all are the Criteo-shape kernels with their own front end.
// Reference: model/deepFM.py:23-31 (x = [dense | emb], sigmoid(c0*dnn + c1*fm)).
#include <stdlib.h>

#include <type_traits>

#include "embed_fm_body.hpp"
#include "rs_common.hpp"

namespace rs {

// Fused DeepFM forward: gather + FM + DNN tower + head, one launch.
template <int KV, int KIND>
__global__ __launch_bounds__(16 * 64) void deepfm_fused(EmbedFmArgs a, MlpArgs t) {
  embed_fm_body<KV, 1, 16, KIND, true, 1>(a, &t, blockIdx.x);
}
// ... with the field metadata by value (rs_deepfm_fwd_hm; see embed_fm_mfma_ka)
template <int KV, int KIND>
__global__ __launch_bounds__(16 * 64) void deepfm_fused_ka(EmbedFmArgs a, MlpArgs t, FieldMeta m) {
  embed_fm_body<KV, 1, 16, KIND, true, 1, false, true>(a, &t, blockIdx.x, &m);
}

// ---- Fused DeepFM with split wave roles (deepfm_ws; rs_deepfm_fwd_hm at the
// Criteo shape: k = 16, 26 fields, 1..16 dense features, a first hidden layer
// of 241..256 units).  The tower's first layer is the bulk of the MFMA work
// and only needs each field's 16 columns of the tile, so it need not wait for
// the whole gather: waves 0..7 LOAD — ids, then the rows in two bursts
// (fields 0..15, 16..25) into the LDS tile, the FM partial tiles on the way,
// the dense block — and count each burst in an LDS counter; waves 8..15
// COMPUTE layer 0 (two 16-column output tiles each, k-groups in arrival
// order: the dense group first, then the fields) with their weight ring
// streaming from the start and waiting only on the counters.  Their vector
// memory queue holds weights only, so no row load sits in front of a weight
// wait.  The FM partials of the loaders meet by the last-wave finish; layers
// 1.. run as mlp_tower_tile on all 16 waves.  Every spin is bounded.
constexpr int WS_NL = 8;

// A logic error must neither hang the kernel nor pass silently: a wait that
// gives up raises RS_FLAG_TIMEOUT in the launch's error flag (the host layer
// then raises RSError instead of returning the outputs) and the kernel runs
// on to its end, so every wave still reaches every barrier and the grid drains.
__device__ __forceinline__ void lds_wait_ge(int* p, int v, int* err) {
  for (int spins = 0; __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < v; ++spins) {
    if (spins > (1 << 22)) {
      if ((threadIdx.x & 63) == 0) flag_error(err, RS_FLAG_TIMEOUT);
      break;
    }
    __builtin_amdgcn_s_sleep(1);
  }
}
__device__ __forceinline__ void lds_signal(int* p) {
  if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(p, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

template <int KIND, int G, int GWA = 0, int GWB = 0>
__global__ __launch_bounds__(16 * 64) void deepfm_ws(EmbedFmArgs a, MlpArgs t, FieldMeta m) {
  typedef Ids<KIND> I;
  constexpr int NW = 16, F = G - 1, MF = (F + WS_NL - 1) / WS_NL;
  static_assert(F <= 32 && MF <= 4, "deepfm_ws: <= 32 fields");
  extern __shared__ float tsm[];
  __shared__ floatx4 lf_acc[WS_NL][64];
  __shared__ floatx4 lf_q[WS_NL][4];
  __shared__ float fmlog[16];
  __shared__ int cnt[4];  // dense k-steps written | loaders past burst 0 | past burst 1 | FM partials in
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int s = lane & 15, kk = lane >> 4;
  const int64_t bt = (int64_t)blockIdx.x * 16 + s;
  const bool valid = bt < a.batch;
  const int64_t b = valid ? bt : a.batch - 1;
  const int RS = t.rs;
  float* par = tsm + 32 * RS + NW * 256;
  floatx4 ring[MLP_R];
  {
    const MlpArgs& a = t;  // MLP_STAMP reads a.dbg (diagnostic hook)
    MLP_STAMP(0);
  }
  if (threadIdx.x < 4) cnt[threadIdx.x] = 0;
  if (w < WS_NL) {
    // ================================ loader
    const int l = w;
    const float w0v = a.w0[0];
    const int dw = l - (WS_NL - a.DB);  // dense k-steps on the last DB loaders (fewest fields)
    const bool has_dense = dw >= 0;
    float dx = 0.f, drec = 0.f, dn = 0.f;
    if (has_dense) {
      const int e = 4 * dw + kk;
      dx = a.dense[b * a.dense_stride + (e < a.nd ? e : 0)];
      const float* rec = a.prep + (int64_t)dw * a.dense_rec;
      drec = rec[lane];
      dn = rec[64 + kk];
    }
    typename I::raw_t rid[MF];
    floatx4 bw[MF];
#pragma unroll
    for (int p = 0; p < MF; ++p) {
      const int c = l + WS_NL * p;
      bw[p] = floatx4{0.f, 0.f, 0.f, 0.f};
      if (c < F) {
        rid[p] = I::load(a.ids, b * a.id_stride + c);
        if (s <= a.kfm) bw[p] = *reinterpret_cast<const floatx4*>(a.prep + a.field_base + (int64_t)c * a.field_rec + lane * 4);
      }
    }
    // burst 0's rows go out before the barrier (round 5: the bias-block copy
    // that used to sit here — two dependent L2 trips — moved to the compute
    // waves, which wait for the rows anyway)
    floatx4 xs0[2];
    bool ok0[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int c = l + WS_NL * q;
      ok0[q] = false;
      if (q < MF && c < F) {
        int64_t id;
        ok0[q] = I::decode(rid[q], m.voc[c], id);
        xs0[q] = __builtin_nontemporal_load(reinterpret_cast<const floatx4*>(a.table + (m.off[c] + id) * 16) + kk);
      }
    }
    __syncthreads();  // the counters start at 0 (the compute waves pass the same barrier)
    floatx4 ac[4];  // four accumulation chains (MFMA tp into chain tp)
#pragma unroll
    for (int c = 0; c < 4; ++c) ac[c] = floatx4{0.f, 0.f, 0.f, 0.f};
    float qn = 0.f;
    if (has_dense) {  // the dense group of the tile: dense columns + the zero padding up to 16
      const int e = 4 * dw + kk;
      const float x = e < a.nd ? dx : 0.f;
      ac[0] = mfma16x16x4(x, drec, ac[0]);
      qn = fmaf(x * x, dn, qn);
      tsm[s * RS + F * 16 + e] = x;
      lds_signal(&cnt[0]);
    }
    float nrm[MF][4];
#pragma unroll
    for (int p = 0; p < MF; ++p)
#pragma unroll
      for (int tp = 0; tp < 4; ++tp) nrm[p][tp] = row16_sum(s < a.kfm ? bw[p][tp] * bw[p][tp] : 0.f);
    bool bad = false;
#pragma unroll
    for (int burst = 0; burst < 2; ++burst) {
      floatx4 xs[2];
      bool ok[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int p = 2 * burst + q, c = l + WS_NL * p;
        if (burst == 0) {
          xs[q] = xs0[q];
          ok[q] = ok0[q];
          continue;
        }
        ok[q] = false;
        if (p < MF && c < F) {
          int64_t id;
          ok[q] = I::decode(rid[p], m.voc[c], id);
          xs[q] = __builtin_nontemporal_load(reinterpret_cast<const floatx4*>(a.table + (m.off[c] + id) * 16) + kk);
        }
      }
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int p = 2 * burst + q, c = l + WS_NL * p;
        if (p < MF && c < F) {
          bad |= !ok[q];
          const floatx4 x = ok[q] ? xs[q] : floatx4{0.f, 0.f, 0.f, 0.f};
          *reinterpret_cast<floatx4*>(tsm + s * RS + c * 16 + 4 * kk) = x;
#pragma unroll
          for (int tp = 0; tp < 4; ++tp) {
            ac[tp] = mfma16x16x4(x[tp], bw[p][tp], ac[tp]);
            qn = fmaf(x[tp] * x[tp], nrm[p][tp], qn);
          }
        }
      }
#ifdef RS_DIAG_STAMPS
      if (!(burst == 1 && (a.ablate & 32)))  // diagnostic knob: burst 1 never signalled (the timeout test)
#endif
      lds_signal(&cnt[1 + burst]);
      {
        const MlpArgs& a = t;
        MLP_STAMP(2 + burst);  // diagnostic hook: this loader's burst in
      }
    }
    if (__any(bad && valid) && lane == 0) flag_error(a.err);
    // FM: last-wave finish over the loaders' partial tiles (wave order)
    floatx4 acc;
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = (ac[0][i] + ac[1][i]) + (ac[2][i] + ac[3][i]);
    lf_acc[l][lane] = acc;
    qn += __shfl_xor(qn, 16);
    qn += __shfl_xor(qn, 32);
    if (lane < 16) reinterpret_cast<float*>(&lf_q[l][0])[lane] = qn;
    int old = 0;
    if (lane == 0) old = __hip_atomic_fetch_add(&cnt[3], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
    old = __builtin_amdgcn_readfirstlane(old);
    if (old == WS_NL - 1) {
      floatx4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ww = 0; ww < WS_NL; ++ww) {
        const floatx4 pv = lf_acc[ww][lane];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] += pv[i];
      }
      const floatx4 q4 = lf_q[s < WS_NL ? s : 0][kk];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float tt = s < a.kfm ? v[i] * v[i] : 0.f;
        if (s < WS_NL) tt -= q4[i];
        float ll = s == a.kfm ? v[i] : 0.f;
        tt = row16_sum(tt);
        ll = row16_sum(ll);
        const float fm = (ll + w0v) + 0.5f * tt;
        const int64_t bb = (int64_t)blockIdx.x * 16 + 4 * kk + i;
        if (s == 0) {
          fmlog[4 * kk + i] = fm;
          if (bb < a.batch && a.logit) a.logit[bb] = fm;
        }
      }
    }
  } else {
    // ================================ layer 0 compute
    const int c8 = w - WS_NL;
    const floatx4* W0 = reinterpret_cast<const floatx4*>(t.prep + t.off[0]) + lane + (int64_t)c8 * G * 64;
    const floatx4* W1 = W0 + (int64_t)WS_NL * G * 64;  // output tile c8 + 8
    // k-group order: the dense group (G - 1) first, then fields 0 .. F-1
    auto grp = [](int i) { return i == 0 ? G - 1 : i - 1; };
    floatx4 r0[3], r1[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      r0[u] = W0[(int64_t)grp(u) * 64];
      r1[u] = W1[(int64_t)grp(u) * 64];
    }
    __syncthreads();  // the counters start at 0
    // the bias / alpha block -> LDS for the layers after the first (visible
    // at the tail's first barrier); this layer's epilogue reads its 4 values
    // per lane from global memory, so no hand-off among the compute waves
    for (int i = threadIdx.x - WS_NL * 64; i < t.ptot; i += (NW - WS_NL) * 64) par[i] = t.prep[t.wtot + i];
    const int ecol0 = 16 * c8 + s, ecol1 = ecol0 + 16 * WS_NL;
    const float* pb = t.prep + t.wtot + t.poff[0];
    const float eb0 = pb[ecol0], eb1 = pb[ecol1], ea0 = pb[t.Np[0] + ecol0], ea1 = pb[t.Np[0] + ecol1];
    const float* ap = tsm + s * RS + 4 * kk;
    // two output tiles, two chains each (MFMA j of a group into chain j & 1)
    floatx4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0, acc0b = acc0, acc1b = acc0;
    lds_wait_ge(&cnt[0], a.DB, a.err);
    // one k-group: MFMAs of ring slot U, then the slot refilled 3 groups ahead
    auto step = [&](int i, auto U) {
      constexpr int u = decltype(U)::value;
      const floatx4 av = *reinterpret_cast<const floatx4*>(ap + 16 * grp(i));
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < 4; j += 2) {
        acc0 = mfma16x16x4(av[j], r0[u][j], acc0);
        acc1 = mfma16x16x4(av[j], r1[u][j], acc1);
        acc0b = mfma16x16x4(av[j + 1], r0[u][j + 1], acc0b);
        acc1b = mfma16x16x4(av[j + 1], r1[u][j + 1], acc1b);
      }
      const int nx = i + 3 < G ? i + 3 : G - 1;
      r0[u] = W0[(int64_t)grp(nx) * 64];
      r1[u] = W1[(int64_t)grp(nx) * 64];
      __builtin_amdgcn_sched_barrier(0);
    };
    using U0 = std::integral_constant<int, 0>;
    using U1 = std::integral_constant<int, 1>;
    using U2 = std::integral_constant<int, 2>;
    auto wait_burst = [&](int which) {
      lds_wait_ge(&cnt[1 + which], WS_NL, a.err);  // fields 0..15 / 16.. in the tile
      const MlpArgs& a = t;
      MLP_STAMP(2 + which);  // diagnostic hook: burst seen
    };
    constexpr int B1 = 1 + 2 * WS_NL;  // first group of the second burst
    if (t.unroll) {
      // straight-line (RS_OPT_MLP_UNROLL 1)
#pragma unroll
      for (int i = 0; i < G; ++i) {
        if (i == 1) wait_burst(0);
        if (i == B1) wait_burst(1);
        if (i % 3 == 0) step(i, U0{});
        else if (i % 3 == 1) step(i, U1{});
        else step(i, U2{});
      }
    } else {
      // compact loops (three groups a trip, ring slots fixed per position):
      // straight-line code of this length runs at instruction-fetch speed
      // (every 64-B line a miss, the cache is cold each launch: DESIGN 10)
      static_assert((B1 - 2) % 3 == 0 && (G - 1 - B1) % 3 == 0, "deepfm_ws: group / ring phase");
      step(0, U0{});
      wait_burst(0);
      int i = 1;
#pragma unroll 1
      for (; i + 2 < B1; i += 3) {
        step(i, U1{});
        step(i + 1, U2{});
        step(i + 2, U0{});
      }
      step(i, U1{});  // i = B1 - 1
      wait_burst(1);
#pragma unroll 1
      for (i = B1; i + 2 < G; i += 3) {
        step(i, U2{});
        step(i + 1, U0{});
        step(i + 2, U1{});
      }
      step(i, U2{});  // i = G - 1
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      acc0[i] += acc0b[i];
      acc1[i] += acc1b[i];
    }
    float* out = tsm + 16 * RS;  // layer 0 -> buf1
    with_act(t.act[0], [&](auto A) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 4 * kk + r;
        out[row * RS + ecol0] = mlp_act_c<decltype(A)::value>(acc0[r] + eb0, ea0);
        out[row * RS + ecol1] = mlp_act_c<decltype(A)::value>(acc1[r] + eb1, ea1);
      }
    });
  }
  {
    const MlpArgs& a = t;
    MLP_STAMP(1);  // loader: rows + FM done; compute wave: layer 0 done
  }
  if constexpr (GWA > 0) {
    // the split-K tail (mlp_tail_splitk) at the DeepFM widths: layer 1's whole slice of this wave
    if constexpr (GWA == 8 && GWB == 2) {
      mlp_tail_run<NW>(t, tsm, (int64_t)blockIdx.x * 16, fmlog);
    } else {
      floatx4 wr[GWA];
      mlp_tail_fetch<GWA>(t, 1, wr);
      mlp_tail_splitk<NW, GWA, GWB>(t, tsm, (int64_t)blockIdx.x * 16, wr, fmlog, 1);
    }
  } else {
    {  // layer 1's first weights (this wave's first item of it, if any)
      const int T1 = t.Np[1] >> 4, G1 = t.Kp[1] >> 4;
      const int S1 = mlp_slices(T1, G1, NW);
      if (w < T1 * S1) {
        const MlpItem it = mlp_item(w, T1, G1, S1);
        mlp_ring_fill(ring, reinterpret_cast<const floatx4*>(t.prep + t.off[1]) + lane + (int64_t)it.t * G1 * 64,
                      it.g0, it.g1);
      }
    }
    mlp_tower_tile<NW>(t, tsm, (int64_t)blockIdx.x * 16, ring, fmlog, 1);
  }
}

// ---- Fused DeepFM, every wave on layer 0 (deepfm_all; RS_OPT_DEEPFM_KERNEL 2
// / 3 = weight ring 3 / 4 k-groups deep) at the Criteo shape (k 16, 26 fields,
// 1..16 dense features, a 256-unit first layer).  deepfm_ws ran layer 0 on 8
// of the 16 waves (2 per SIMD, ~48 cycles per MFMA per SIMD) while the other
// 8 gathered; here all 16 waves both gather and compute, one 16-column output
// tile of layer 0 each (4 waves per SIMD share the matrix pipe), and nothing
// spins (two workgroup barriers publish the two row bursts):
//   * front end (the headline kernel's recipe): only the ids of the wave's
//     fields c0 = w, c1 = w + 16 (< 26) and the dense features of waves
//     12..15 go out before the first burst (row c0 of every wave); weights,
//     FM fragments and the bias block follow it;
//   * row c0 -> LDS tile + its FM partial (MFMA against the packed [v | w1]
//     image, q = sum x^2 |v|^2 on the VALU), the dense group written by waves
//     12..15 -> barrier A -> the second burst (row c1) requested, layer 0
//     over the dense group and fields 0..15 with row c1 stored under them ->
//     barrier B -> fields 16..25 (every load unconditional, every wait the
//     compiler's counted one).  Requesting c1 only after barrier A: barrier A
//     waits for 8.4 MB of row lines instead of 13.6 (7.5k vs 11.4k cycles);
//   * the 16 FM partial tiles meet in LDS (fixed wave order); every wave then
//     finishes one sample's FM logit; layers 1.. run as the split-K tail
//     (mlp_tail_splitk) at the DeepFM widths, else as mlp_tower_tile.
// Reference: model/deepFM.py:23-31, layer/interaction.py:40-46 (DNN),
// :106-114 (FM), layer/core.py:273-280 (lookup).
template <int KIND, int G, int RD, int GWA = 0, int GWB = 0>
__global__ __launch_bounds__(16 * 64) void deepfm_all(EmbedFmArgs a, MlpArgs t, FieldMeta m) {
  typedef Ids<KIND> I;
  constexpr int NW = 16, F = G - 1;
  static_assert(F > 16 && F <= 32, "deepfm_all: 17..32 fields (two per wave at most)");
  static_assert(RD == 3 || RD == 4, "deepfm_all: weight ring 3 or 4 k-groups deep");
  extern __shared__ float tsm[];
  __shared__ floatx4 fm_acc[NW][64];  // FM partial tile of each wave
  __shared__ float fm_q[NW][16];      // sum_i x_i^2 |v_i|^2 partial of each wave, per sample
  __shared__ float fmlog[16];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int s = lane & 15, kk = lane >> 4;
  const int64_t bt = (int64_t)blockIdx.x * 16 + s;
  const bool valid = bt < a.batch;
  const int64_t b = valid ? bt : a.batch - 1;  // padded lanes recompute the last sample
  const int RS = t.rs;
  float* par = tsm + 32 * RS + NW * 256;
  {
    const MlpArgs& a = t;
    MLP_STAMP(0);
  }
  // ---- front end: ids (+ the dense features of waves 12..15), then row c0
  const int c0 = w, c1 = w + 16 < F ? w + 16 : w;  // (waves past F-16: c1 re-reads c0, unused)
  const bool two = w + 16 < F;                     // wave-uniform
  const typename I::raw_t rid0 = I::load(a.ids, b * a.id_stride + c0);
  const typename I::raw_t rid1 = I::load(a.ids, b * a.id_stride + c1);
  const int dw = w - (NW - 4);                  // FM dense k-step of waves 12..15 (they also write the dense group)
  const bool has_dense = dw >= 0 && dw < a.DB;  // wave-uniform
  const int dwc = dw < 0 ? 0 : (dw < a.DB ? dw : 0);
  const int de = 4 * dwc + kk;
  const float dxv = a.dense[b * a.dense_stride + (de < a.nd ? de : 0)];
  int64_t id0, id1;
  const bool ok0 = I::decode(rid0, m.voc[c0], id0);
  const bool ok1 = I::decode(rid1, m.voc[c1], id1);
  const floatx4 x0 = __builtin_nontemporal_load(reinterpret_cast<const floatx4*>(a.table + (m.off[c0] + id0) * 16) + kk);
  const floatx4* x1p = reinterpret_cast<const floatx4*>(a.table + (m.off[c1] + id1) * 16) + kk;
  // ---- behind the first burst: layer-0 weights of output tile w (k-groups in
  // the order dense (G-1), 0, 1, ..), the FM fragments, the bias / alpha block
  const floatx4* W0 = reinterpret_cast<const floatx4*>(t.prep + t.off[0]) + lane + (int64_t)w * G * 64;
  auto grp = [](int i) { return i == 0 ? G - 1 : i - 1; };
  floatx4 ring[RD];
#pragma unroll
  for (int u = 0; u < RD; ++u) ring[u] = W0[(int64_t)grp(u) * 64];
  const float* drec = a.prep + (int64_t)dwc * a.dense_rec;
  const float drv = drec[lane], dnv = drec[64 + kk];
  const floatx4 bw0 = *reinterpret_cast<const floatx4*>(a.prep + a.field_base + (int64_t)c0 * a.field_rec + lane * 4);
  const floatx4 bw1 = *reinterpret_cast<const floatx4*>(a.prep + a.field_base + (int64_t)c1 * a.field_rec + lane * 4);
  const float w0v = a.w0[0];
  const int npar = t.ptot;
  const int pi = threadIdx.x < npar ? threadIdx.x : 0;
  const float pv = t.prep[t.wtot + pi];
  bool bad = !ok0 || (two && !ok1);
  // ---- layer 0, four chains (MFMA j of a k-group into chain j), ring slot i % RD
  MacAcc<4> L0;
  const float* ap = tsm + s * RS + 4 * kk;
  // A fragments one k-group ahead inside a segment (the LDS latency hides
  // behind the previous group's MFMAs); a segment's first read is issued
  // after its barrier (seg_start)
  floatx4 an = {0.f, 0.f, 0.f, 0.f};
  auto seg_start = [&](int i) { an = *reinterpret_cast<const floatx4*>(ap + 16 * grp(i)); };
  auto step = [&](int i, auto U) {
    constexpr int u = decltype(U)::value;
    const floatx4 av = an;
    if (i != 16 && i + 1 < G) an = *reinterpret_cast<const floatx4*>(ap + 16 * grp(i + 1));  // 16: last before barrier B
    __builtin_amdgcn_sched_barrier(0);
    L0.mac4(av, ring[u]);
    if (i + RD < G) ring[u] = W0[(int64_t)grp(i + RD) * 64];
    __builtin_amdgcn_sched_barrier(0);
  };
  auto step_i = [&](int i) {
    switch (i % RD) {
      case 0: step(i, std::integral_constant<int, 0>{}); break;
      case 1: step(i, std::integral_constant<int, 1>{}); break;
      case 2: step(i, std::integral_constant<int, 2>{}); break;
      default: step(i, std::integral_constant<int, (RD > 3 ? 3 : 0)>{}); break;
    }
  };
  // ---- FM partials: the dense k-step, then each field as its row lands
  floatx4 fa = {0.f, 0.f, 0.f, 0.f};
  float qn = 0.f;
  if (dw >= 0) {
    // the tile's dense group (columns F*16 .. F*16+15, zero past nd), and the FM's dense k-step
    const int e = 4 * dw + kk;
    const float x = e < a.nd ? dxv : 0.f;
    tsm[s * RS + F * 16 + e] = x;
    if (has_dense) {
      fa = mfma16x16x4(x, drv, fa);
      qn = fmaf(x * x, dnv, qn);
    }
  }
  float n0[4], n1[4];
#pragma unroll
  for (int tp = 0; tp < 4; ++tp) {
    n0[tp] = row16_sum(s < a.kfm ? bw0[tp] * bw0[tp] : 0.f);
    n1[tp] = row16_sum(s < a.kfm ? bw1[tp] * bw1[tp] : 0.f);
  }
  if (threadIdx.x < npar) par[pi] = pv;
  auto put_row = [&](int c, const floatx4& xr, bool ok, const floatx4& bw, const float (&nr)[4]) {
    const floatx4 x = ok ? xr : floatx4{0.f, 0.f, 0.f, 0.f};
    *reinterpret_cast<floatx4*>(tsm + s * RS + c * 16 + 4 * kk) = x;
#pragma unroll
    for (int tp = 0; tp < 4; ++tp) {
      fa = mfma16x16x4(x[tp], bw[tp], fa);
      qn = fmaf(x[tp] * x[tp], nr[tp], qn);
    }
  };
  put_row(c0, x0, ok0, bw0, n0);
  __syncthreads();  // A: fields 0..15 (one per wave), the dense group, the bias / alpha block in LDS
  {
    const MlpArgs& a = t;
    MLP_STAMP(2);
  }
  // the second burst (unconditional: waves past F-16 re-read their first row)
  const floatx4 x1 = __builtin_nontemporal_load(x1p);
  __builtin_amdgcn_sched_barrier(0);
  // the dense group and fields 0..15: k-groups 0..16; row c1 lands under the first nine
  seg_start(0);
#pragma unroll
  for (int i = 0; i <= 16; ++i) {
    step_i(i);
    if (i == 8) {
      if (two) put_row(c1, x1, ok1, bw1, n1);
      // the wave's FM partial tile (its fields + dense k-step) for the combine
      fm_acc[w][lane] = fa;
      qn += __shfl_xor(qn, 16);
      qn += __shfl_xor(qn, 32);
      if (lane < 16) fm_q[w][lane] = qn;
      if (__any(bad && valid) && lane == 0) flag_error(a.err);
    }
  }
  __syncthreads();  // B: fields 16..F-1 in the tile, the FM partials in LDS
  {
    const MlpArgs& a = t;
    MLP_STAMP(3);
  }
  // FM logit of sample w (wave = sample, lane = column < 16): its 16 wave
  // partials added in wave order — the reads go out before the last layer-0
  // groups and are summed after them; wave index ww doubles as the q column.
  float fmv[NW];
  {
    const int ln = (w >> 2) * 16 + s, r = w & 3;
#pragma unroll
    for (int ww = 0; ww < NW; ++ww) fmv[ww] = fm_acc[ww][ln][r];
  }
  const float fq = fm_q[s][w];
  seg_start(17);
#pragma unroll
  for (int i = 17; i < G; ++i) step_i(i);
  const floatx4 acc0 = L0.sum();
  // layer 1's weights: the split-K tail's whole slice, or the ring's first groups
  constexpr bool TAIL = GWA > 0;
  floatx4 wr[TAIL ? GWA : 1];
  floatx4 tring[MLP_R];
  if constexpr (TAIL) {
    mlp_tail_fetch<GWA>(t, 1, wr);
  } else {
    const int T1 = t.Np[1] >> 4, G1 = t.Kp[1] >> 4;
    const int S1 = mlp_slices(T1, G1, NW);
    if (w < T1 * S1) {
      const MlpItem it = mlp_item(w, T1, G1, S1);
      mlp_ring_fill(tring, reinterpret_cast<const floatx4*>(t.prep + t.off[1]) + lane + (int64_t)it.t * G1 * 64,
                    it.g0, it.g1);
    }
  }
  {
    float* out = tsm + 16 * RS;  // layer 0 -> buf1
    const int col = 16 * w + s;
    const float bc = par[t.poff[0] + col], ac = par[t.poff[0] + t.Np[0] + col];  // registers before the stores
    with_act(t.act[0], [&](auto A) {
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(4 * kk + r) * RS + col] = mlp_act_c<decltype(A)::value>(acc0[r] + bc, ac);
    });
  }
  {
    float v = 0.f;
#pragma unroll
    for (int ww = 0; ww < NW; ++ww) v += fmv[ww];
    float tq = (s < a.kfm ? v * v : 0.f) - fq;
    float lin = s == a.kfm ? v : 0.f;
    tq = row16_sum(tq);
    lin = row16_sum(lin);
    const float fm = (lin + w0v) + 0.5f * tq;
    if (lane == 0) {
      fmlog[w] = fm;
      const int64_t bb = (int64_t)blockIdx.x * 16 + w;
      if (bb < a.batch && a.logit) a.logit[bb] = fm;
    }
  }
  {
    const MlpArgs& a = t;
    MLP_STAMP(1);
  }
  if constexpr (TAIL) {
    if constexpr (GWA == 8 && GWB == 2) mlp_tail_dispatch<NW>(t, tsm, (int64_t)blockIdx.x * 16, wr, fmlog, 1);
    else mlp_tail_splitk<NW, GWA, GWB>(t, tsm, (int64_t)blockIdx.x * 16, wr, fmlog, 1);
  }
  else mlp_tower_tile<NW>(t, tsm, (int64_t)blockIdx.x * 16, tring, fmlog, 1);
}

// ------------------------------------------------------- launch helpers
static bool deepfm_geom(int nd, int n_fields, int k, int kfm, int n_layers, const int* dims, FmGeom& fg,
                        MlpGeom& mg) {
  if (nd < 0 || n_fields < 1 || n_fields > 128 || kfm < 1 || (k != 8 && k != 16)) return false;
  fg = fm_geom(nd, n_fields, k, kfm);
  if (!fg.mfma || fg.NT != 1) return false;
  if (!mlp_geom(n_layers, dims, mg)) return false;
  // static LDS of the embed part (<= 37 KB) + the tower's dynamic LDS
  return dims[0] == nd + n_fields * k && dims[n_layers] == 1 && mg.lds <= 120 * 1024;
}

// deepfm_ws covers: kernel-argument metadata, k = 16, 26 fields, 13..16 dense
// features (one k-group of dense + padding, written whole by the 4 dense
// loaders), a first hidden layer of 241..256
// units (16 output tiles: two per compute wave), >= 2 layers whose second has
// >= 8 output tiles (its items start on the loader waves)
static bool deepfm_ws_ok(const EmbedFmArgs& a, const MlpArgs& t, const FieldMeta* hm, int KV) {
  return hm && KV == 4 && a.F == 26 && a.nd >= 13 && a.nd <= 16 && a.DB == 4 && t.L >= 2 &&
         t.Np[0] == 256 && t.Kp[0] == 16 * (a.F + 1) && (t.Np[1] >> 4) >= WS_NL &&
         opt(RS_OPT_DEEPFM_KERNEL) == 0;
}

// deepfm_all covers the same shapes as deepfm_ws (every wave owns one of the
// 16 output tiles of the 256-unit first layer and at most two of the fields)
static bool deepfm_all_ok(const EmbedFmArgs& a, const MlpArgs& t, const FieldMeta* hm, int KV) {
  return hm && KV == 4 && a.F == 26 && a.nd >= 1 && a.nd <= 16 && a.DB <= 4 && t.L >= 2 && t.Np[0] == 256 &&
         t.Kp[0] == 16 * (a.F + 1) && t.ptot <= 1024 && opt(RS_OPT_DEEPFM_KERNEL) >= 2;
}

template <int KV, int KIND>
static void launch_deepfm(const EmbedFmArgs& a, const MlpArgs& t, size_t lds, hipStream_t st,
                          const FieldMeta* hm) {
  const unsigned grid = (unsigned)((a.batch + 15) / 16);
  if constexpr (KV == 4) {
    if (deepfm_all_ok(a, t, hm, KV)) {
      // the split-K tail at the DeepFM widths (256 -> 128 -> 64 -> 1: 8 + 2
      // k-groups per wave), the one-role tail for other towers
      int gwa = 0, gwb = 0;
      const bool tail = mlp_tail_ok(t.Np, t.Kp, t.N, t.L, 1, gwa, gwb) && gwa == 8 && gwb == 2;
      const bool ring4 = opt(RS_OPT_DEEPFM_KERNEL) == 3;
      if (tail && ring4) launch_lds<deepfm_all<KIND, 27, 4, 8, 2>>(grid, 16 * 64, lds, st, a, t, *hm);
      else if (tail) launch_lds<deepfm_all<KIND, 27, 3, 8, 2>>(grid, 16 * 64, lds, st, a, t, *hm);
      else launch_lds<deepfm_all<KIND, 27, 3>>(grid, 16 * 64, lds, st, a, t, *hm);
      return;
    }
    if (deepfm_ws_ok(a, t, hm, KV)) {
      // layers 1.. as the split-K tail at the DeepFM widths (256 -> 128 -> 64 -> 1), else mlp_tower_tile
      int gwa = 0, gwb = 0;
      if (mlp_tail_ok(t.Np, t.Kp, t.N, t.L, 1, gwa, gwb) && gwa == 8 && gwb == 2)
        launch_lds<deepfm_ws<KIND, 27, 8, 2>>(grid, 16 * 64, lds, st, a, t, *hm);
      else launch_lds<deepfm_ws<KIND, 27>>(grid, 16 * 64, lds, st, a, t, *hm);
      return;
    }
  }
  // the kernarg body is built lean for at most 16 dense k-steps (nd <= 64):
  // its dense loop is compiled out (embed_fm_body: dense_small = KA || ...)
  if (hm && a.F <= 32 && a.DB <= 16) launch_lds<deepfm_fused_ka<KV, KIND>>(grid, 16 * 64, lds, st, a, t, *hm);
  else launch_lds<deepfm_fused<KV, KIND>>(grid, 16 * 64, lds, st, a, t);
}

}  // namespace rs

using namespace rs;

extern "C" int rs_deepfm_fused_ok(int nd, int n_fields, int k, int kfm, int n_layers, const int* dims) {
  FmGeom fg;
  MlpGeom mg;
  return dims && deepfm_geom(nd, n_fields, k, kfm, n_layers, dims, fg, mg) ? 1 : 0;
}

static int deepfm_run(const void* ids, int id_kind, int64_t id_stride, const float* dense, int64_t dense_stride,
                      int nd, const float* table, const int64_t* field_offsets, const int64_t* field_vocab,
                      int n_fields, int k, const float* fm_prepared, const float* w0, int kfm, int n_layers,
                      const int* dims, const int* acts, const float* mlp_prepared, float c0, float c1, float* out,
                      float* fm_logit, int64_t batch, int* err_flag, rs_stream_t stream, const FieldMeta* hm) {
  if (batch == 0) return RS_OK;  // empty batch: nothing to launch (null data pointers allowed)
  FmGeom fg;
  MlpGeom mg;
  RS_REQUIRE(dims && acts, "rs_deepfm_fwd: null dims/acts");
  RS_REQUIRE(deepfm_geom(nd, n_fields, k, kfm, n_layers, dims, fg, mg),
             "rs_deepfm_fwd: unsupported shape (see rs_deepfm_fused_ok)");
  RS_REQUIRE(batch >= 0 && ids && table && field_offsets && field_vocab && fm_prepared && w0 && mlp_prepared && out,
             "rs_deepfm_fwd: null pointer");
  RS_REQUIRE(nd == 0 || dense, "rs_deepfm_fwd: dense is null");
  RS_REQUIRE(id_kind >= RS_ID_I32 && id_kind <= RS_ID_F32, "rs_deepfm_fwd: bad id_kind");
  RS_REQUIRE((uintptr_t)table % 16 == 0, "rs_deepfm_fwd: table must be 16-B aligned");
  MlpArgs t{};
  RS_REQUIRE(mlp_fill_args(mg, acts, mlp_prepared, t), "rs_deepfm_fwd: bad activation");
  t.y = out;
  t.ys = 1;
  t.head = 1;
  t.c0 = c0;
  t.c1 = c1;
  t.M = batch;
  t.dbg = mlp_diag_dbg();
  EmbedFmArgs a = fm_args(ids, id_stride, dense, dense_stride, nd, table, field_offsets, field_vocab, n_fields, k,
                          fm_prepared, w0, kfm, fm_logit, nullptr, batch, err_flag);
  set_geom(a, fg);
#ifdef RS_DIAG_STAMPS
  a.ablate = getenv("RS_ABLATE") ? atoi(getenv("RS_ABLATE")) : 0;  // 32: deepfm_ws never signals burst 1
#endif
  hipStream_t st = as_stream(stream);
  with_id_kind(id_kind, [&](auto K) {
    constexpr int KIND = decltype(K)::value;
    if (fg.KV == 2) launch_deepfm<2, KIND>(a, t, mg.lds, st, hm);
    else launch_deepfm<4, KIND>(a, t, mg.lds, st, hm);
  });
  return launch_status("rs_deepfm_fwd");
}

extern "C" int rs_deepfm_fwd(const void* ids, int id_kind, int64_t id_stride, const float* dense,
                             int64_t dense_stride, int nd, const float* table, const int64_t* field_offsets,
                             const int64_t* field_vocab, int n_fields, int k, const float* fm_prepared,
                             const float* w0, int kfm, int n_layers, const int* dims, const int* acts,
                             const float* mlp_prepared, float c0, float c1, float* out, float* fm_logit,
                             int64_t batch, int* err_flag, rs_stream_t stream) {
  return deepfm_run(ids, id_kind, id_stride, dense, dense_stride, nd, table, field_offsets, field_vocab, n_fields, k,
                    fm_prepared, w0, kfm, n_layers, dims, acts, mlp_prepared, c0, c1, out, fm_logit, batch, err_flag,
                    stream, nullptr);
}

extern "C" int rs_deepfm_fwd_hm(const void* ids, int id_kind, int64_t id_stride, const float* dense,
                                int64_t dense_stride, int nd, const float* table, const int64_t* field_offsets,
                                const int64_t* field_vocab, const int64_t* field_offsets_host,
                                const int64_t* field_vocab_host, int n_fields, int k, const float* fm_prepared,
                                const float* w0, int kfm, int n_layers, const int* dims, const int* acts,
                                const float* mlp_prepared, float c0, float c1, float* out, float* fm_logit,
                                int64_t batch, int* err_flag, rs_stream_t stream) {
  RS_REQUIRE(batch == 0 || (field_offsets_host && field_vocab_host), "rs_deepfm_fwd_hm: host metadata missing");
  const bool use = n_fields <= 32 && batch > 0;
  const FieldMeta m = field_meta(field_offsets_host, field_vocab_host, use ? n_fields : 0);
  return deepfm_run(ids, id_kind, id_stride, dense, dense_stride, nd, table, field_offsets, field_vocab, n_fields, k,
                    fm_prepared, w0, kfm, n_layers, dims, acts, mlp_prepared, c0, c1, out, fm_logit, batch, err_flag,
                    stream, use ? &m : nullptr);
}
