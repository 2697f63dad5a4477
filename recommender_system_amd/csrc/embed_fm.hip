// embed_fm.hip — the fused embedding lookup + FM second-order kernels: the
// K-split / kernarg / preload / stream kernels around embed_fm_body
// (embed_fm_body.hpp) and the generic fallback.  The other kernel families of
// the same body live in shard_fm.hip (sharded owner / pipe) and deepfm.hip
// (fused DeepFM); the plain gather and the one-hot FM in embed_gather.hip.
//
// Reference semantics:
//   EmbedLayer.call            algorithm/deep_learning/layer/core.py:273-280
//   DeepFM x = [dense | emb]   algorithm/deep_learning/model/deepFM.py:24-26
//   FMLayer.call               algorithm/deep_learning/layer/interaction.py:106-114
//
// Headline kernel: embed_fm_mfma — one launch does ids -> rows -> FM logit.
//   * A workgroup owns 16 samples (one MFMA row tile) and NW waves split the
//     contraction dimension d = nd + F*k round-robin by field (K-split).
//   * Lane l of a wave is sample s = l&15 and k-slot kk = l>>4: for field c it
//     loads k/4 consecutive floats of the sample's row (k=16: one float4, so a
//     wave-instruction reads 16 whole 64-B rows), which are its A-operand
//     values for the field's k/4 MFMA k-steps (k order permuted per field;
//     the packed B image from rs_fm_prepare uses the same permutation).
//   * s = x@v and the linear term x@w1 come out of v_mfma_f32_16x16x4_f32
//     (B columns 0..kfm-1 = v, column kfm = w1); the second-order correction
//     sum_f (x^2@v^2)_f = sum_i x_i^2 * |v_i|^2 is a per-lane FMA with the row
//     norms packed beside B, reduced across the 4 k-slots by two lane swaps
//     (v_permlane16_swap / v_permlane32_swap: no LDS round trip).
//   * Partial tiles of the NW waves are summed through LDS ([sample][column]
//     [wave]: a thread's 16 partials in four 16-B reads); wave 0 finishes
//     logit = (x@w1 + w0) + 0.5*(sum_f s_f^2 - sum_i x_i^2 |v_i|^2).
#include <stdlib.h>

#include <type_traits>

#include "embed_fm_body.hpp"
#include "rs_common.hpp"

namespace rs {

__device__ __forceinline__ float fm_bval(const float* w1, const float* v, int d, int kfm, int e, int colg) {
  if (e >= d) return 0.f;
  if (colg < kfm) return v[(int64_t)e * kfm + colg];
  if (colg == kfm) return w1[e];
  return 0.f;
}

__device__ __forceinline__ float fm_rownorm(const float* v, int d, int kfm, int e) {
  if (e >= d) return 0.f;
  float n = 0.f;
  for (int f = 0; f < kfm; ++f) {
    const float t = v[(int64_t)e * kfm + f];
    n = fmaf(t, t, n);
  }
  return n;
}

__global__ void fm_prepare_mfma(const float* __restrict__ w1, const float* __restrict__ v, int nd, int F,
                                int k, int kfm, int KV, int NT, int DB, int64_t dense_rec,
                                int64_t field_rec, int64_t field_base, int64_t size,
                                float* __restrict__ out) {
  const int d = nd + F * k;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < size;
       idx += (int64_t)gridDim.x * blockDim.x) {
    float val;
    if (idx < field_base) {
      const int t = (int)(idx / dense_rec);
      const int r = (int)(idx % dense_rec);
      if (r < NT * 64) {
        const int nt = r / 64, lane = r % 64;
        const int e = 4 * t + (lane >> 4);
        val = (e < nd) ? fm_bval(w1, v, d, kfm, e, nt * 16 + (lane & 15)) : 0.f;
      } else {
        const int e = 4 * t + (r - NT * 64);
        val = (e < nd) ? fm_rownorm(v, d, kfm, e) : 0.f;
      }
    } else {
      const int64_t j = idx - field_base;
      const int c = (int)(j / field_rec);
      const int r = (int)(j % field_rec);
      if (r < NT * 64 * KV) {
        const int nt = r / (64 * KV), rem = r % (64 * KV);
        const int lane = rem / KV, tp = rem % KV;
        const int e = nd + c * k + KV * (lane >> 4) + tp;
        val = fm_bval(w1, v, d, kfm, e, nt * 16 + (lane & 15));
      } else {
        const int r2 = r - NT * 64 * KV;
        const int e = nd + c * k + KV * (r2 / KV) + (r2 % KV);
        val = fm_rownorm(v, d, kfm, e);
      }
    }
    out[idx] = val;
  }
}

__global__ void fm_prepare_generic(const float* __restrict__ w1, const float* __restrict__ v, int d, int kfm,
                                   float* __restrict__ out) {
  const int64_t n = (int64_t)d * (kfm + 2);
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n;
       idx += (int64_t)gridDim.x * blockDim.x) {
    float val;
    if (idx < d) val = w1[idx];
    else if (idx < (int64_t)d * (kfm + 1)) val = v[idx - d];
    else val = fm_rownorm(v, d, kfm, (int)(idx - (int64_t)d * (kfm + 1)));
    out[idx] = val;
  }
}

template <int KV, int NT, int NW, int KIND, int MC, bool PF = false>
__global__ __launch_bounds__(NW * 64) void embed_fm_mfma(EmbedFmArgs a) {
  embed_fm_body<KV, NT, NW, KIND, false, MC, PF>(a, nullptr, blockIdx.x);
}

// the field metadata by value (rs_embed_fm_fwd_hm): each wave loads its own
// fields' ids and reads (offset, vocab) through scalar kernarg loads — no LDS
// id tile, no barrier, no per-wave metadata loads from one hot L2 line
// (ID1: both passes' ids in one load — embed_fm_body.hpp; the single launch takes it for integer ids, KV * NT <= 8)
template <int KV, int NT, int NW, int KIND, bool PF, int FC = 0, int KFMC = 0, int NDC = -1, bool ID1 = false>
__global__ __launch_bounds__(NW * 64) void embed_fm_mfma_ka(EmbedFmArgs a, FieldMeta m) {
  embed_fm_body<KV, NT, NW, KIND, false, 1, PF, true, FC, KFMC, NDC, false, ID1>(a, nullptr, blockIdx.x, &m);
}

// ---- the kernarg kernels with their hot arguments preloaded (RS_OPT_EMBED_FM_KERNEL 5;
// EmbedFmCold and hot_cold_args in embed_fm_body.hpp say how and why)
// host side of hot_cold_args' compile-time geometry: does the run-time geometry equal the specialised
// kernels' compile-time one?  (false: the launcher takes the generic kernel)
template <int KV, int NT, int FC, int KFMC, int NDC>
static bool ct_geom_matches(const EmbedFmArgs& a) {
  constexpr FmGeom G = fm_geom(NDC, FC, 4 * KV, KFMC);
  return G.mfma && G.KV == KV && G.NT == NT && a.F == FC && a.kfm == KFMC && a.nd == NDC && a.k == 4 * KV &&
         a.DB == G.DB && a.dense_rec == G.dense_rec && a.field_rec == G.field_rec && a.field_base == G.field_base;
}

// The one specialised shape (Criteo / the headline: 26 fields, FM width 10,
// 13 dense features, k 16): 1 = this is it and the compile-time geometry
// holds (the specialised kernels run), 0 = another shape, -1 = the shape but
// not the geometry (the generic kernels run; rs_embed_fm_ct_geom reports it)
static int headline_spec(const EmbedFmArgs& a) {
  if (a.F != 26 || a.kfm != 10 || a.nd != 13 || a.k != 16) return 0;
  return ct_geom_matches<4, 1, 26, 10, 13>(a) ? 1 : -1;
}

template <int KV, int NT, int NW, int KIND, bool PF, int FC = 0, int KFMC = 0, int NDC = -1, bool ID1 = false>
__global__ __launch_bounds__(NW * 64) void embed_fm_mfma_kp(const float* prep, const void* ids, int64_t id_stride,
                                                            int64_t batch, const float* dense, int64_t dense_stride,
                                                            const float* table, EmbedFmCold c, FieldMeta m) {
  const EmbedFmArgs a = hot_cold_args<KV, NT, FC, KFMC, NDC>(prep, ids, id_stride, batch, dense, dense_stride, table, c);
  embed_fm_body<KV, NT, NW, KIND, false, 1, PF, true, FC, KFMC, NDC, true, ID1>(a, nullptr, blockIdx.x, &m);
}

// S consecutive batches in ONE launch (rs_embed_fm_fwd_hm_stream): workgroup
// g runs the kernarg kernel's body on tile g % tpb of batch g / tpb (batch-
// major dispatch order) — the same instantiation and tile arithmetic as the
// per-batch launch, so every batch's logits are bit-identical to
// rs_embed_fm_fwd_hm's; batch s's ids / dense / logit start at the given
// per-batch strides; the last batch may be shorter (its own tile count).
// One build serves both values of the entry point's min_blocks: the second
// __launch_bounds__ argument is a minimum of waves per EU (SIMD), not of
// workgroups per CU, and a 1,024-thread workgroup already places 4 waves on
// every SIMD, so asking for 1 or 2 compiled to the same code.
struct StreamArgs {
  int tpb, S;
  int64_t ids_bstride_bytes, dense_bstride, logit_bstride, last_batch;
};
template <int KV, int NT, int KIND, int FC = 0, int KFMC = 0, int NDC = -1>
__global__ __launch_bounds__(16 * 64) void embed_fm_stream_ka(EmbedFmArgs a, FieldMeta m, StreamArgs sa) {
  const int s = blockIdx.x / sa.tpb, tile = blockIdx.x - s * sa.tpb;
  EmbedFmArgs b = a;
  b.ids = static_cast<const char*>(a.ids) + s * sa.ids_bstride_bytes;
  b.dense = a.dense + s * sa.dense_bstride;
  b.logit = a.logit + s * sa.logit_bstride;
  if (s == sa.S - 1) b.batch = sa.last_batch;
  if ((int64_t)tile * 16 >= b.batch) return;  // a shorter last batch: fewer tiles (uniform exit)
  embed_fm_body<KV, NT, 16, KIND, false, 1, true, true, FC, KFMC, NDC>(b, nullptr, tile, &m);
}
// ... with the hot arguments preloaded (embed_fm_mfma_kp); the batch index
// and strides are cold, so only the B-fragment loads go out ahead of them
template <int KV, int NT, int KIND, int FC = 0, int KFMC = 0, int NDC = -1>
__global__ __launch_bounds__(16 * 64) void embed_fm_stream_kp(const float* prep, const void* ids, int64_t id_stride,
                                                              int64_t batch, const float* dense, int64_t dense_stride,
                                                              const float* table, EmbedFmCold c, FieldMeta m,
                                                              StreamArgs sa) {
  const int s = blockIdx.x / sa.tpb, tile = blockIdx.x - s * sa.tpb;
  EmbedFmArgs b = hot_cold_args<KV, NT, FC, KFMC, NDC>(prep, ids, id_stride, batch, dense, dense_stride, table, c);
  b.ids = static_cast<const char*>(ids) + s * sa.ids_bstride_bytes;
  b.dense = dense + s * sa.dense_bstride;
  b.logit = c.logit + s * sa.logit_bstride;
  if (s == sa.S - 1) b.batch = sa.last_batch;
  if ((int64_t)tile * 16 >= b.batch) return;  // a shorter last batch: fewer tiles (uniform exit)
  embed_fm_body<KV, NT, 16, KIND, false, 1, true, true, FC, KFMC, NDC, true>(b, nullptr, tile, &m);
}

// Generic fallback (any k / kfm): one 256-thread workgroup per sample.
__device__ __forceinline__ float block_sum(float v, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  float t = 0.f;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += red[i];
  return t;
}

template <int KIND>
__global__ __launch_bounds__(256) void embed_fm_generic(EmbedFmArgs a) {
  typedef Ids<KIND == 3 ? 0 : KIND> I;
  __shared__ int64_t rows[1024];
  __shared__ float red[4];
  const int64_t b = blockIdx.x;
  const int d = a.nd + a.F * a.k;
  const float* w1 = a.prep;
  const float* v = a.prep + d;
  const float* nsq = a.prep + (int64_t)d * (a.kfm + 1);
  for (int c = threadIdx.x; c < a.F; c += blockDim.x) {
    int64_t row = b * a.F + c;
    if constexpr (KIND != 3) {
      int64_t id;
      if (I::decode(I::load(a.ids, b * a.id_stride + c), a.vocab[c], id)) row = a.offs[c] + id;
      else { row = -1; flag_error(a.err); }
    }
    rows[c] = row;
  }
  __syncthreads();
  auto xval = [&](int e) -> float {
    if (e < a.nd) return a.dense[b * a.dense_stride + e];
    const int c = (e - a.nd) / a.k, j = (e - a.nd) % a.k;
    const int64_t r = rows[c];
    return r >= 0 ? a.table[r * a.k + j] : 0.f;
  };
  float lin = 0.f, q = 0.f;
  for (int e = threadIdx.x; e < d; e += blockDim.x) {
    const float x = xval(e);
    lin = fmaf(x, w1[e], lin);
    q = fmaf(x * x, nsq[e], q);
    if (a.x_out) a.x_out[b * d + e] = x;
  }
  lin = block_sum(lin, red);
  q = block_sum(q, red);
  float ss = 0.f;
  for (int f = 0; f < a.kfm; ++f) {
    float p = 0.f;
    for (int e = threadIdx.x; e < d; e += blockDim.x) p = fmaf(xval(e), v[(int64_t)e * a.kfm + f], p);
    p = block_sum(p, red);
    ss = fmaf(p, p, ss);
  }
  if (threadIdx.x == 0) a.logit[b] = (lin + a.w0[0]) + 0.5f * (ss - q);
}

// ------------------------------------------------------- launch helpers
// Which form of the kernarg kernels a launch takes (RS_OPT_EMBED_FM_KERNEL):
// 4 = EmbedFmArgs by value (embed_fm_mfma_ka / embed_fm_stream_ka), 5 = the
// hot arguments preloaded (embed_fm_mfma_kp / embed_fm_stream_kp); any other
// value: the default below, decided by the A/B in DESIGN.md 4.1 (5.97 ->
// 5.63 us per launch at B 4096, 5.36 -> 4.82 at 2048, bit-identical;
// profiles/ab_kernarg_preload_{4096,2048}.jsonl).
constexpr bool kKernargPreloadDefault = true;
static bool kernarg_preload() {
  const int v = opt(RS_OPT_EMBED_FM_KERNEL);
  return v == 5 || (v != 4 && kKernargPreloadDefault);
}

template <int KV, int NT, int KIND>
static void launch_embed_fm3(const EmbedFmArgs& a, hipStream_t st, const FieldMeta* hm) {
  // 16 waves per 16-sample tile (measured against 4, 8 and 13 waves), one
  // field slot per wave and pass: the headline's 26 fields take two passes
  // (16 + 10), 6.05 us per launch against 6.54 with both in one pass (2 slots
  // per wave) — the second pass's row requests queue behind a shorter first
  // wave of 256 rows per CU.  More than 32 fields: 2 slots per pass.
  const int grid = (int)((a.batch + 15) / 16);
  // several tiles per CU: prefetch the first passes' B fragments (PF) and
  // use fewer waves per tile, so more tiles share a CU (one field slot per
  // wave and pass): 8 waves up to 1024 tiles, 4 beyond (scripts/ab A/B,
  // graph slots: 13.0 -> 11.4 us at B 12288, 14.5 -> 13.5 at 16384, 27.0 ->
  // 22.9 at 32768, 50.7 -> 42.7 at 65536; profiles/r3_ab_nw*.json)
  // host field metadata given (rs_embed_fm_fwd_hm), up to 2 tiles per CU:
  // the kernarg-metadata kernel (6.92 -> 6.50 us at B 4096, 6.10 -> 5.78 at
  // 2048; profiles/r3_ab_kernarg_meta_{4096,2048}.json)
  // with the ids loaded per wave, the first passes' B fragments beside them
  // pay at 4096 too (6.61 -> 6.39 us, profiles/r3_ab_kernarg_pf_4096.json);
  // above 512 tiles the device-metadata kernels stay faster (14.26 vs 13.48
  // us at 16384, 47.5 vs 42.6 at 65536, still 14.34 vs 13.54 / 47.8 vs 42.6
  // with both passes' ids requested together; profiles/r3_ab_kernarg_*)
  // 16 waves (13: 6.20 us, 9: 6.78 vs 5.76 at 4096; profiles/r3_ab_kernarg_waves_4096.json)
  // (the kernarg kernel is built lean: at most 2 x 16 fields, 16 dense k-steps,
  // no x output — its straight-line code runs from a cold instruction cache)
  if constexpr (KIND != 3) {  // (rows already gathered: never the kernarg kernels — none instantiated)
    if (hm && a.F <= 32 && grid <= 512 && a.DB <= 16 && !a.x_out) {
      // (round 5: the ids through 16 scalar loads per wave and a lane select
      // chain, off the vector memory queue, ran 7.08 vs 6.12 us per launch,
      // bit-identical — profiles/r5_ab_scalar_ids.json; not kept)
      const bool pl = kernarg_preload();
      const EmbedFmCold c = cold_args(a);
      if constexpr (KV == 4 && NT == 1 && KIND != 2) {
        // the Criteo / headline shape (its compile-time geometry checked: a
        // mismatch would take the generic kernel, which reads the run-time one)
        if (headline_spec(a) == 1) {
          if (pl)
            embed_fm_mfma_kp<KV, NT, 16, KIND, true, 26, 10, 13, true><<<grid, 16 * 64, 0, st>>>(
                a.prep, a.ids, a.id_stride, a.batch, a.dense, a.dense_stride, a.table, c, *hm);
          else embed_fm_mfma_ka<KV, NT, 16, KIND, true, 26, 10, 13, true><<<grid, 16 * 64, 0, st>>>(a, *hm);
          return;
        }
      }
      // (any other shape: the merged id load too — 5.55 -> 5.41 us at 26 fields, FM width 8 — for integer
      // ids and where embed_fm_body runs its two-pass schedule, PRE: KV * NT <= 8.  Longer rows, k 64 or
      // k 32 with two column tiles, take the pass-at-a-time loop, which loads each pass's ids on its own.)
      constexpr bool ID1 = KIND != 2 && KV * NT <= 8;
      if (pl)
        embed_fm_mfma_kp<KV, NT, 16, KIND, true, 0, 0, -1, ID1><<<grid, 16 * 64, 0, st>>>(
            a.prep, a.ids, a.id_stride, a.batch, a.dense, a.dense_stride, a.table, c, *hm);
      else embed_fm_mfma_ka<KV, NT, 16, KIND, true, 0, 0, -1, ID1><<<grid, 16 * 64, 0, st>>>(a, *hm);
      return;
    }
  }
  if (a.F <= 32 && grid > 1024) embed_fm_mfma<KV, NT, 4, KIND, 1, true><<<grid, 4 * 64, 0, st>>>(a);
  else if (a.F <= 32 && grid > 512) embed_fm_mfma<KV, NT, 8, KIND, 1, true><<<grid, 8 * 64, 0, st>>>(a);
  else if (a.F <= 32) embed_fm_mfma<KV, NT, 16, KIND, 1><<<grid, 16 * 64, 0, st>>>(a);
  else embed_fm_mfma<KV, NT, 16, KIND, 0><<<grid, 16 * 64, 0, st>>>(a);
}

template <int KIND>
static void launch_embed_fm_k(const EmbedFmArgs& a, int KV, int NT, hipStream_t st,
                              const FieldMeta* hm = nullptr) {
  with_kv(KV, [&](auto kv) {
    constexpr int V = decltype(kv)::value;
    if (NT == 1) launch_embed_fm3<V, 1, KIND>(a, st, hm);
    else launch_embed_fm3<V, 2, KIND>(a, st, hm);
  });
}

// kind: RS_ID_* or 3 (rows already gathered)
static int run_embed_fm(EmbedFmArgs a, const FmGeom& g, int kind, hipStream_t st, const char* what,
                        const FieldMeta* hm = nullptr) {
  if (a.batch == 0) return RS_OK;
  if (g.mfma) {
    set_geom(a, g);
    if (a.F == 0) {
      // dense-only (FMLayer on x): no field loop runs, any instantiation works
      launch_embed_fm_k<3>(a, 4, g.NT, st);
    } else if (kind == 3) {
      launch_embed_fm_k<3>(a, g.KV, g.NT, st);
    } else if (launch_embed_fm_tiles(a, g, kind, opt(RS_OPT_EMBED_FM_KERNEL), st)) {
      // the persistent tile kernels (embed_fm_tiles.hip), when selected and the shape fits
    } else {
      with_id_kind(kind, [&](auto K) { launch_embed_fm_k<decltype(K)::value>(a, g.KV, g.NT, st, hm); });
    }
  } else {
    if (a.F > 1024) {
      set_error("%s: generic FM path supports at most 1024 fields", what);
      return RS_ERR_UNSUPPORTED;
    }
    if (kind == 3 || a.F == 0) embed_fm_generic<3><<<(unsigned)a.batch, 256, 0, st>>>(a);
    else with_id_kind(kind, [&](auto K) {
      embed_fm_generic<decltype(K)::value><<<(unsigned)a.batch, 256, 0, st>>>(a);
    });
  }
  return launch_status(what);
}

}  // namespace rs

using namespace rs;

extern "C" int64_t rs_fm_prepared_size(int nd, int n_fields, int k, int kfm) {
  if (nd < 0 || n_fields < 0 || kfm < 1 || (n_fields > 0 && k < 1)) return -1;
  return fm_geom(nd, n_fields, k, kfm).size;
}

extern "C" int rs_embed_fm_ct_geom(int nd, int n_fields, int k, int kfm) {
  if (nd < 0 || n_fields < 0 || kfm < 1 || (n_fields > 0 && k < 1)) return 0;
  const FmGeom g = fm_geom(nd, n_fields, k, kfm);
  if (!g.mfma) return 0;
  EmbedFmArgs a{};
  a.nd = nd;
  a.F = n_fields;
  a.k = k;
  a.kfm = kfm;
  set_geom(a, g);
  return headline_spec(a);
}

extern "C" int rs_fm_prepare(const float* w1, const float* v, int nd, int n_fields, int k, int kfm,
                             float* prepared, rs_stream_t stream) {
  RS_REQUIRE(w1 && v && prepared, "rs_fm_prepare: null pointer");
  RS_REQUIRE(nd >= 0 && n_fields >= 0 && kfm >= 1 && (n_fields == 0 || k >= 1), "rs_fm_prepare: bad shape");
  const FmGeom g = fm_geom(nd, n_fields, k, kfm);
  RS_REQUIRE(g.d > 0, "rs_fm_prepare: empty feature vector");
  hipStream_t st = as_stream(stream);
  if (g.mfma) {
    fm_prepare_mfma<<<grid_for(g.size, 256), 256, 0, st>>>(w1, v, nd, n_fields, k, kfm, g.KV, g.NT, g.DB,
                                                           g.dense_rec, g.field_rec, g.field_base, g.size,
                                                           prepared);
  } else {
    fm_prepare_generic<<<grid_for(g.size, 256), 256, 0, st>>>(w1, v, g.d, kfm, prepared);
  }
  return launch_status("rs_fm_prepare");
}

// argument checks shared by rs_embed_fm_fwd and rs_embed_fm_fwd_hm (`what`: the entry point's name)
static int check_embed_fm(const char* what, const void* ids, int id_kind, const float* dense, int nd,
                          const float* table, const int64_t* field_offsets, const int64_t* field_vocab, int n_fields,
                          int k, const float* prepared, const float* w0, int kfm, const float* logit, int64_t batch) {
  RS_REQUIRE(batch >= 0 && nd >= 0 && n_fields >= 0 && kfm >= 1, "%s: bad shape", what);
  RS_REQUIRE(prepared && w0 && logit, "%s: null pointer", what);
  RS_REQUIRE(nd == 0 || dense, "%s: dense is null", what);
  RS_REQUIRE(n_fields == 0 || (ids && table && field_offsets && field_vocab && k >= 1), "%s: sparse inputs missing",
             what);
  RS_REQUIRE(id_kind >= RS_ID_I32 && id_kind <= RS_ID_F32, "%s: bad id_kind", what);
  RS_REQUIRE(k % 4 != 0 || (uintptr_t)table % 16 == 0, "%s: table must be 16-B aligned", what);
  return RS_OK;
}

extern "C" int rs_embed_fm_fwd(const void* ids, int id_kind, int64_t id_stride, const float* dense,
                               int64_t dense_stride, int nd, const float* table, const int64_t* field_offsets,
                               const int64_t* field_vocab, int n_fields, int k, const float* prepared,
                               const float* w0, int kfm, float* logit, float* x_out, int64_t batch,
                               int* err_flag, rs_stream_t stream) {
  if (batch == 0) return RS_OK;  // empty batch: nothing to launch (null data pointers allowed)
  if (const int rc = check_embed_fm("rs_embed_fm_fwd", ids, id_kind, dense, nd, table, field_offsets, field_vocab,
                                    n_fields, k, prepared, w0, kfm, logit, batch))
    return rc;
  const EmbedFmArgs a = fm_args(ids, id_stride, dense, dense_stride, nd, table, field_offsets, field_vocab, n_fields, k,
                                prepared, w0, kfm, logit, x_out, batch, err_flag);
  return run_embed_fm(a, fm_geom(nd, n_fields, k, kfm), id_kind, as_stream(stream), "rs_embed_fm_fwd");
}

extern "C" int rs_embed_fm_fwd_hm(const void* ids, int id_kind, int64_t id_stride, const float* dense,
                                  int64_t dense_stride, int nd, const float* table, const int64_t* field_offsets,
                                  const int64_t* field_vocab, const int64_t* field_offsets_host,
                                  const int64_t* field_vocab_host, int n_fields, int k, const float* prepared,
                                  const float* w0, int kfm, float* logit, float* x_out, int64_t batch,
                                  int* err_flag, rs_stream_t stream) {
  if (batch == 0) return RS_OK;
  RS_REQUIRE(field_offsets_host && field_vocab_host, "rs_embed_fm_fwd_hm: host metadata missing");
  const int variant = opt(RS_OPT_EMBED_FM_KERNEL);
  if (n_fields > 32 || (variant >= 1 && variant <= 3))
    return rs_embed_fm_fwd(ids, id_kind, id_stride, dense, dense_stride, nd, table, field_offsets, field_vocab,
                           n_fields, k, prepared, w0, kfm, logit, x_out, batch, err_flag, stream);
  if (const int rc = check_embed_fm("rs_embed_fm_fwd_hm", ids, id_kind, dense, nd, table, field_offsets, field_vocab,
                                    n_fields, k, prepared, w0, kfm, logit, batch))
    return rc;
  const FieldMeta m = field_meta(field_offsets_host, field_vocab_host, n_fields);
  const EmbedFmArgs a = fm_args(ids, id_stride, dense, dense_stride, nd, table, field_offsets, field_vocab, n_fields, k,
                                prepared, w0, kfm, logit, x_out, batch, err_flag);
  return run_embed_fm(a, fm_geom(nd, n_fields, k, kfm), id_kind, as_stream(stream), "rs_embed_fm_fwd_hm", &m);
}

// S consecutive batch requests of `batch` samples each (the last one
// `last_batch`), batch s's ids at ids + s * ids_batch_stride elements, dense
// at dense + s * dense_batch_stride, logits at logit + s * logit_batch_stride:
// one launch, each batch's logits bit-identical to rs_embed_fm_fwd_hm's on
// that batch alone.  The kernarg-metadata kernel's shapes only (k 16 / 8 / 4,
// kfm <= 15, <= 32 fields, <= 16 dense k-steps, int32 / int64 ids, batch <=
// 8192, no x output); min_blocks: 1 or 2, both the same kernel (see
// embed_fm_stream_ka).
extern "C" int rs_embed_fm_fwd_hm_stream(const void* ids, int id_kind, int64_t id_stride, int64_t ids_batch_stride,
                                         const float* dense, int64_t dense_stride, int64_t dense_batch_stride,
                                         int nd, const float* table, const int64_t* field_offsets_host,
                                         const int64_t* field_vocab_host, int n_fields, int k,
                                         const float* prepared, const float* w0, int kfm, float* logit,
                                         int64_t logit_batch_stride, int64_t batch, int n_batches,
                                         int64_t last_batch, int min_blocks, int* err_flag, rs_stream_t stream) {
  if (n_batches == 0 || batch == 0) return RS_OK;
  RS_REQUIRE(n_batches > 0 && batch > 0 && last_batch > 0 && last_batch <= batch && batch <= 8192 && nd >= 0 &&
                 nd <= 64 && n_fields >= 1 && n_fields <= 32 && kfm >= 1 && kfm <= 15 &&
                 (k == 4 || k == 8 || k == 16) && (min_blocks == 1 || min_blocks == 2),
             "rs_embed_fm_fwd_hm_stream: unsupported shape");
  RS_REQUIRE(id_kind == RS_ID_I32 || id_kind == RS_ID_I64, "rs_embed_fm_fwd_hm_stream: int32 / int64 ids only");
  RS_REQUIRE(ids && table && prepared && w0 && logit && (nd == 0 || dense) && field_offsets_host &&
                 field_vocab_host,
             "rs_embed_fm_fwd_hm_stream: null pointer");
  RS_REQUIRE((uintptr_t)table % 16 == 0, "rs_embed_fm_fwd_hm_stream: table must be 16-B aligned");
  RS_REQUIRE(ids_batch_stride >= batch * id_stride && dense_batch_stride >= (nd ? batch * dense_stride : 0) &&
                 logit_batch_stride >= batch,
             "rs_embed_fm_fwd_hm_stream: batches overlap");
  const int64_t tpb = (batch + 15) / 16;
  RS_REQUIRE(tpb * n_batches < (1ll << 31), "rs_embed_fm_fwd_hm_stream: too many tiles");
  const FieldMeta m = field_meta(field_offsets_host, field_vocab_host, n_fields);
  // (no device metadata, no x output: the kernarg kernels read neither)
  EmbedFmArgs a = fm_args(ids, id_stride, dense, dense_stride, nd, table, nullptr, nullptr, n_fields, k, prepared, w0,
                          kfm, logit, nullptr, batch, err_flag);
  set_geom(a, fm_geom(nd, n_fields, k, kfm));
  StreamArgs sa{(int)tpb, n_batches, ids_batch_stride * (id_kind == RS_ID_I64 ? 8 : 4), dense_batch_stride,
                logit_batch_stride, last_batch};
  const unsigned grid = (unsigned)(tpb * n_batches);
  hipStream_t st = as_stream(stream);
  const bool pl = kernarg_preload();
  const EmbedFmCold c = cold_args(a);
  auto go = [&](auto kv, auto kind) {
    constexpr int KV = decltype(kv)::value, KIND = decltype(kind)::value;
    const dim3 gr(grid), bl(16 * 64);
    // (specialised shape, preloaded hot arguments) -> instantiation
    auto run = [&](auto spec) {
      constexpr int FC = decltype(spec)::value ? 26 : 0, KC = FC ? 10 : 0, NC = FC ? 13 : -1;
      if (pl)
        embed_fm_stream_kp<KV, 1, KIND, FC, KC, NC><<<gr, bl, 0, st>>>(a.prep, a.ids, a.id_stride, a.batch, a.dense,
                                                                      a.dense_stride, a.table, c, m, sa);
      else embed_fm_stream_ka<KV, 1, KIND, FC, KC, NC><<<gr, bl, 0, st>>>(a, m, sa);
    };
    if constexpr (KV == 4) {
      // the headline shape, as the single launch (geometry checked as there)
      if (headline_spec(a) == 1) {
        run(std::true_type());
        return;
      }
    }
    run(std::false_type());
  };
  auto by_kind = [&](auto kv) {
    if (id_kind == RS_ID_I64) go(kv, std::integral_constant<int, 1>());
    else go(kv, std::integral_constant<int, 0>());
  };
  if (k == 16) by_kind(std::integral_constant<int, 4>());
  else if (k == 8) by_kind(std::integral_constant<int, 2>());
  else by_kind(std::integral_constant<int, 1>());
  return launch_status("rs_embed_fm_fwd_hm_stream");
}

extern "C" int rs_rows_fm_fwd(const float* emb, const float* dense, int64_t dense_stride, int nd, int n_fields,
                              int k, const float* prepared, const float* w0, int kfm, float* logit, int64_t batch,
                              rs_stream_t stream) {
  if (batch == 0) return RS_OK;  // empty batch: nothing to launch (null data pointers allowed)
  RS_REQUIRE(batch >= 0 && nd >= 0 && n_fields >= 0 && kfm >= 1, "rs_rows_fm_fwd: bad shape");
  RS_REQUIRE(prepared && w0 && logit && (n_fields == 0 || emb) && (nd == 0 || dense),
             "rs_rows_fm_fwd: null pointer");
  RS_REQUIRE(k % 4 != 0 || (uintptr_t)emb % 16 == 0, "rs_rows_fm_fwd: emb must be 16-B aligned");
  const FmGeom g = fm_geom(nd, n_fields, k, kfm);
  EmbedFmArgs a{};
  a.dense = dense;
  a.dense_stride = dense_stride;
  a.nd = nd;
  a.table = emb;
  a.F = n_fields;
  a.k = k;
  a.prep = prepared;
  a.w0 = w0;
  a.kfm = kfm;
  a.logit = logit;
  a.batch = batch;
  return run_embed_fm(a, g, 3, as_stream(stream), "rs_rows_fm_fwd");
}

extern "C" int rs_fm_fwd(const float* x, int64_t x_stride, int n, const float* prepared, const float* w0, int kfm,
                         float* logit, int64_t batch, rs_stream_t stream) {
  if (batch == 0) return RS_OK;  // empty batch: nothing to launch (null data pointers allowed)
  RS_REQUIRE(x && prepared && w0 && logit, "rs_fm_fwd: null pointer");
  RS_REQUIRE(n >= 1 && kfm >= 1 && batch >= 0, "rs_fm_fwd: bad shape");
  const FmGeom g = fm_geom(n, 0, 0, kfm);
  EmbedFmArgs a{};
  a.dense = x;
  a.dense_stride = x_stride;
  a.nd = n;
  a.F = 0;
  a.k = 0;
  a.prep = prepared;
  a.w0 = w0;
  a.kfm = kfm;
  a.logit = logit;
  a.batch = batch;
  return run_embed_fm(a, g, 3, as_stream(stream), "rs_fm_fwd");
}

#ifdef RS_DIAG_STAMPS
// Ceiling probe: sum 64-B rows at given row indices (4 lanes per row, one
// float4 each) with different cache-policy bits on the row load.
template <int MODE>
__device__ __forceinline__ floatx4 probe_load(const float* p) {
  if constexpr (MODE == 0) {
    return *reinterpret_cast<const floatx4*>(p);
  } else if constexpr (MODE == 1) {
    return __builtin_nontemporal_load(reinterpret_cast<const floatx4*>(p));
  } else {
    floatx4 v;
    if constexpr (MODE == 2) asm volatile("global_load_dwordx4 %0, %1, off sc1\n s_waitcnt vmcnt(0)" : "=v"(v) : "v"(p) : "memory");
    else if constexpr (MODE == 3) asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1 nt\n s_waitcnt vmcnt(0)" : "=v"(v) : "v"(p) : "memory");
    else asm volatile("global_load_dwordx4 %0, %1, off sc0\n s_waitcnt vmcnt(0)" : "=v"(v) : "v"(p) : "memory");
    return v;
  }
}
template <int MODE>
__global__ __launch_bounds__(256) void diag_gather_sum(const float* __restrict__ table,
                                                      const int64_t* __restrict__ rows, int64_t n, float* out) {
  float acc = 0.f;
  // MODE 5: nontemporal with the MFMA A-operand lane layout of embed_fm_mfma
  // (lane l reads chunk l>>4 of row l&15: the 4 lanes of a row are 16 apart)
  const int lane = threadIdx.x & 63;
  const int q = MODE == 5 ? lane >> 4 : threadIdx.x & 3;
  const int64_t quad = MODE == 5 ? (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * 16 + (lane & 15)
                                 : ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 2;
  const int64_t nquads = ((int64_t)gridDim.x * blockDim.x) >> 2;
  for (int64_t i = quad; i < n; i += nquads) {
    const floatx4 v = probe_load<MODE == 5 ? 1 : MODE>(table + rows[i] * 16 + 4 * q);
    acc += v[0] + v[1] + v[2] + v[3];
  }
  if (acc == 12345.678f) out[blockIdx.x] = acc;  // keep the loads live, never true
}
extern "C" int rs_diag_gather_sum(const float* table, const int64_t* rows, int64_t n, int grid, float* out,
                                  int mode, rs_stream_t stream) {
  hipStream_t st = as_stream(stream);
  switch (mode) {
    case 0: diag_gather_sum<0><<<grid, 256, 0, st>>>(table, rows, n, out); break;
    case 1: diag_gather_sum<1><<<grid, 256, 0, st>>>(table, rows, n, out); break;
    case 2: diag_gather_sum<2><<<grid, 256, 0, st>>>(table, rows, n, out); break;
    case 3: diag_gather_sum<3><<<grid, 256, 0, st>>>(table, rows, n, out); break;
    case 5: diag_gather_sum<5><<<grid, 256, 0, st>>>(table, rows, n, out); break;
    default: diag_gather_sum<4><<<grid, 256, 0, st>>>(table, rows, n, out); break;
  }
  return launch_status("rs_diag_gather_sum");
}

// Cache-policy probe: U unrolled 16-B loads per lane in flight (4 lanes per
// 64-B row), issued by inline asm with the given policy bits and waited for
// together; POL 0 plain, 1 nt, 2 sc1, 3 sc0 sc1, 4 sc0 sc1 nt, 5 sc1 nt, 6 sc0,
// 7 sc0 nt.
#define RS_PROBE_ASM(bits) asm volatile("global_load_dwordx4 %0, %1, off " bits : "=v"(v[u]) : "v"(p[u]) : "memory")
template <int POL>
__global__ __launch_bounds__(256) void diag_policy_sum(const float* __restrict__ table, const int64_t* __restrict__ rows,
                                                       int64_t n, float* out) {
  constexpr int U = 4;
  float acc = 0.f;
  const int q = threadIdx.x & 3;
  const int64_t quad = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 2;
  const int64_t nquads = ((int64_t)gridDim.x * blockDim.x) >> 2;
  for (int64_t i0 = quad; i0 < n; i0 += U * nquads) {
    const float* p[U];
    floatx4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + u * nquads < n ? i0 + u * nquads : i0;
      p[u] = table + rows[i] * 16 + 4 * q;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if constexpr (POL == 0) RS_PROBE_ASM("");
      else if constexpr (POL == 1) RS_PROBE_ASM("nt");
      else if constexpr (POL == 2) RS_PROBE_ASM("sc1");
      else if constexpr (POL == 3) RS_PROBE_ASM("sc0 sc1");
      else if constexpr (POL == 4) RS_PROBE_ASM("sc0 sc1 nt");
      else if constexpr (POL == 5) RS_PROBE_ASM("sc1 nt");
      else if constexpr (POL == 6) RS_PROBE_ASM("sc0");
      else RS_PROBE_ASM("sc0 nt");
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int u = 0; u < U; ++u) acc += v[u][0] + v[u][1] + v[u][2] + v[u][3];
  }
  if (acc == 12345.678f) out[blockIdx.x] = acc;  // keep the loads live, never true
}
extern "C" int rs_diag_policy_sum(const float* table, const int64_t* rows, int64_t n, int grid, float* out, int pol,
                                  rs_stream_t stream) {
  hipStream_t st = as_stream(stream);
  switch (pol) {
    case 0: diag_policy_sum<0><<<grid, 256, 0, st>>>(table, rows, n, out); break;
    case 1: diag_policy_sum<1><<<grid, 256, 0, st>>>(table, rows, n, out); break;
    case 2: diag_policy_sum<2><<<grid, 256, 0, st>>>(table, rows, n, out); break;
    case 3: diag_policy_sum<3><<<grid, 256, 0, st>>>(table, rows, n, out); break;
    case 4: diag_policy_sum<4><<<grid, 256, 0, st>>>(table, rows, n, out); break;
    case 5: diag_policy_sum<5><<<grid, 256, 0, st>>>(table, rows, n, out); break;
    case 6: diag_policy_sum<6><<<grid, 256, 0, st>>>(table, rows, n, out); break;
    default: diag_policy_sum<7><<<grid, 256, 0, st>>>(table, rows, n, out); break;
  }
  return launch_status("rs_diag_policy_sum");
}

extern "C" int rs_diag_embed_fm_fwd(const void* ids, int id_kind, int64_t id_stride, const float* dense,
                                    int64_t dense_stride, int nd, const float* table, const int64_t* field_offsets,
                                    const int64_t* field_vocab, int n_fields, int k, const float* prepared,
                                    const float* w0, int kfm, float* logit, int64_t batch,
                                    unsigned long long* dbg, rs_stream_t stream) {
  const FmGeom g = fm_geom(nd, n_fields, k, kfm);
  EmbedFmArgs a = fm_args(ids, id_stride, dense, dense_stride, nd, table, field_offsets, field_vocab, n_fields, k,
                          prepared, w0, kfm, logit, nullptr, batch, nullptr);
  a.dbg = dbg;
  a.ablate = getenv("RS_ABLATE") ? atoi(getenv("RS_ABLATE")) : 0;
  if (getenv("RS_DIAG_HM") && n_fields <= 32) {  // the kernarg-metadata kernel (rs_embed_fm_fwd_hm)
    FieldMeta m{};
    (void)hipMemcpy(m.off, field_offsets, n_fields * sizeof(int64_t), hipMemcpyDeviceToHost);
    (void)hipMemcpy(m.voc, field_vocab, n_fields * sizeof(int64_t), hipMemcpyDeviceToHost);
    return run_embed_fm(a, g, id_kind, as_stream(stream), "rs_diag_embed_fm_fwd", &m);
  }
  return run_embed_fm(a, g, id_kind, as_stream(stream), "rs_diag_embed_fm_fwd");
}
#endif
