// embed_fm_body.hpp — the device body of the fused gather + FM kernels, shared
// by the kernel families built around it: the K-split / kernarg / preload /
// stream kernels and embed_fm_generic (embed_fm.hip, where the headline
// kernel's design is described), the sharded owner / pipe parts
// (shard_fm.hip) and the fused DeepFM kernels (deepfm.hip).
#pragma once
#include "embed_fm.hpp"
#include "mlp_tower.hpp"

namespace rs {

// Phase stamps (s_memrealtime, 100 MHz) for the diagnostic library built by
// scripts/build_diag.sh; compiled out of librs_hip.so.
#ifdef RS_DIAG_STAMPS
#define RS_STAMP(i)                                                                          \
  do {                                                                                       \
    __builtin_amdgcn_sched_barrier(0);                                                       \
    if (a.dbg && lane == 0)                                                                  \
      a.dbg[((int64_t)blockIdx.x * NW + w) * 16 + (i)] = __builtin_amdgcn_s_memrealtime();  \
    __builtin_amdgcn_sched_barrier(0);                                                       \
  } while (0)
#define RS_USE(x) asm volatile("" ::"v"(x))
#else
#define RS_STAMP(i) \
  do {              \
  } while (0)
#define RS_USE(x) \
  do {            \
  } while (0)
#endif

// KIND: 0 i32, 1 i64, 2 f32 ids; 3 = rows already gathered (row(b,c) = b*F+c);
// 4 = owner side of the sharded FM (sharded.py, partial protocol): ids are
// int32 LOCAL rows of the owner's shard (-1 = lookup not owned here: a zero
// contribution, not an error), no dense block, and instead of the logit the
// workgroup writes each sample's partial record
//   [s_0 .. s_{kfm-1}, x@w1, sum_i x_i^2 |v_i|^2, 0-pad]   (a.pw floats)
// over the fields it was given; rs_shard_fm_combine finishes the FM.
// TW: fused DeepFM — x goes to an LDS tile ([emb F*k | dense nd | 0-pad],
// row stride tw->rs) instead of x_out, and the DNN tower of mlp_tower.hpp runs
// on it, closed by sigmoid(c0*dnn + c1*fm) (model/deepFM.py:24-30).
// A workgroup owns one 16-sample MFMA row tile.
// FC / KFMC / NDC: the field count, FM width and dense width as compile-time
// constants (0 / 0 / -1: the kernel arguments' run-time values) — the
// headline shape's kernarg and streamed kernels take 26 / 10 / 13
// PL: the caller's hot arguments arrived preloaded in SGPRs (embed_fm_mfma_kp)
// ID1: a wave with two passes loads both passes' ids with ONE instruction
// (the kernarg kernels' single launch, integer ids, only with the two-pass
// schedule PRE below, which splits the load: at one or two tiles per CU
// every vector-memory instruction in front of the rows is on the critical
// path)
template <int KV, int NT, int NW, int KIND, bool TW, int MC = 0, bool PF = false, bool KA = false, int FC = 0,
          int KFMC = 0, int NDC = -1, bool PL = false, bool ID1 = false>
__device__ __forceinline__ void embed_fm_body(const EmbedFmArgs& a, const MlpArgs* tw, const int tile,
                                              const FieldMeta* km = nullptr) {
  static_assert(!ID1 || (KA && PF && !TW && KIND < 2 && MC == 1), "ID1: the kernarg kernels' two-pass schedule only");
  const int aF = FC > 0 ? FC : a.F;        // (compile-time at the specialised shapes)
  const int akfm = KFMC > 0 ? KFMC : a.kfm;
  const int and_ = NDC >= 0 ? NDC : a.nd;
  // MC > 0: field slots per wave and pass (owner kernels with few fields)
  constexpr int MAXC0 = MC > 0 ? MC : 128 / (NW * KV);
  constexpr int MAXC = MAXC0 < 1 ? 1 : (MAXC0 > 8 ? 8 : MAXC0);
  typedef Ids<(KIND >= 3) ? 0 : KIND> I;
  constexpr bool OWNER = KIND == 4;
  // partial tiles of the NW waves for the combine: [sample][column][wave], a
  // thread's NW partials contiguous (16-B reads; the row of CW floats is
  // padded by 4 so they stay 16-B aligned); the fused tower (TW), whose LDS
  // budget counts the old size, keeps [wave][sample][column + 1]
  constexpr int NC = NT * 16;  // columns per sample
  constexpr bool WIDE = !TW && NW % 4 == 0;
  constexpr int CW = NW + 4;
  __shared__ __attribute__((aligned(16))) float cs[WIDE ? 16 * NC * CW : NW * 16 * (NC + 1)];
  __shared__ float qs[NW][16];

  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int s = lane & 15;   // A: sample row of the tile; B/C: column
  const int kk = lane >> 4;  // k-slot
  // (specialised shapes: the row length is the instantiation's, not an argument to wait for)
  const int ak = FC > 0 ? 4 * KV : a.k;
  const int64_t bt = (int64_t)tile * 16 + s;
  const bool valid = bt < a.batch;
  // Padded lanes of the last tile recompute the last sample: an MFMA output
  // row depends only on its own A row, so they never touch valid outputs.
  // (the kernarg kernels are launched for at most 512 tiles: the sample index
  // is an unsigned 32-bit value, so b * stride is a 32 x 64-bit multiply)
  const int64_t b = (KA && !TW) ? (int64_t)(uint32_t)(valid ? (int)bt : (int)a.batch - 1)
                                : (bt < a.batch ? bt : a.batch - 1);
  const int d = and_ + aF * ak;
  // w0 is requested now, not behind the rows (a dependent load at the end;
  // PL: its pointer is a cold argument, so with those — late_args below)
  float w0v = (OWNER || PL) ? 0.f : a.w0[0];

  // four accumulation chains: MFMA tp of a field slot into chain tp & 3,
  // summed below.  Fixed at compile time: the runtime switch this replaced
  // put a scalar branch beside every MFMA and cost 6.01 vs 5.74 us per
  // headline launch (cold instruction cache, profiles/r4_ab_ka_chains_compile_time.json)
  floatx4 ac[NT][4];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int c = 0; c < 4; ++c) ac[nt][c] = floatx4{0.f, 0.f, 0.f, 0.f};
  float qn = 0.f;
  bool bad = false;

  // ---- prologue: everything that does not depend on the ids is issued first
  // (dense features, packed weights, field offsets/vocab), so the kernel's
  // critical path is exactly two dependent memory trips: ids -> rows.
  // A dense block of at most NW k-steps (DeepFM: 13 features = 4 k-steps) is
  // one k-step per wave; wider dense inputs (FMLayer on a plain x) stream.
  // Materialise every kernel argument at entry: one batched s_load instead
  // of lazy per-use kernarg loads (each a dependent K$ round trip).
  // (PL: the hot arguments are in SGPRs already and nothing here may wait for
  // the cold ones — they are materialised behind the id loads, below)
  if constexpr (!PL) {
    asm volatile("" ::"s"(a.ids), "s"(a.id_stride), "s"(a.dense), "s"(a.dense_stride), "s"(a.nd), "s"(a.table),
                 "s"(a.offs), "s"(a.vocab), "s"(aF), "s"(a.k), "s"(a.prep), "s"(akfm));
    asm volatile("" ::"s"(a.batch), "s"(a.DB), "s"(a.dense_rec), "s"(a.field_rec), "s"(a.field_base), "s"(a.x_out),
                 "s"(a.logit), "s"(a.w0), "s"(a.err));
  }
  RS_STAMP(0);
  RS_USE(b);
  RS_STAMP(5);
  if constexpr (TW) {
    const MlpArgs& a = *tw;  // MLP_STAMP reads a.dbg
    MLP_STAMP(0);
  }
  // fused tower: its layer-0 weights, the bias/alpha block and the x tile's
  // zero padding do not depend on the ids; issue them first
  extern __shared__ float tsm[];
  __shared__ float fmlog[TW ? 16 : 1];
  floatx4 ring[TW ? MLP_R : 1];
  const int xrs = TW ? tw->rs : 0;
  if constexpr (TW) {
    mlp_first_fill<NW>(*tw, ring);
    float* par = tsm + 32 * tw->rs + NW * 256;
    for (int i = threadIdx.x; i < tw->ptot; i += NW * 64) par[i] = tw->prep[tw->wtot + i];
    const int d0 = aF * ak + and_, padw = tw->Kp[0] - d0;
    for (int i = threadIdx.x; i < 16 * padw; i += NW * 64) {
      const int r = i / padw;
      tsm[r * xrs + d0 + (i - r * padw)] = 0.f;
    }
  }
  const bool dense_small = KA || a.DB <= NW;  // (the kernarg kernel is launched for DB <= 16 only)
  // Dense k-steps go to the LAST waves: with F = 26 fields over 16 waves the
  // first F - NW waves already carry two fields.
  const int dw = NW - 1 - w;                        // dense k-step of this wave
  const bool has_dense = dense_small && dw < a.DB;  // wave-uniform
  float dx = 0.f, dn = 0.f, drec[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) drec[nt] = 0.f;
  auto load_dense = [&]() {
    if (has_dense) {
      const int e = 4 * dw + kk;
      dx = a.dense[b * a.dense_stride + (e < and_ ? e : 0)];  // masked at use
      const float* rec = a.prep + (int64_t)dw * a.dense_rec;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) drec[nt] = rec[nt * 64 + lane];
      dn = rec[NT * 64 + kk];
    }
  };
  // ---- cooperative id tile: the workgroup's 16 x F ids and the F field
  // (offset, vocab) pairs arrive through coalesced loads into LDS, once per
  // workgroup (instead of 4 redundant lanes per id and one metadata load per
  // wave and field), then one barrier.  Fields beyond FMAX use direct loads.
  constexpr int FMAX = 128;
  __shared__ typename I::raw_t lid[16][FMAX];
  __shared__ int64_t lmeta[2][FMAX];
  // (owner side, KIND 4: the local rows need no field metadata, so every
  // wave loads its own ids — no id tile, no barrier before the rows)
#ifdef RS_DIAG_STAMPS
  const bool coop = !KA && !OWNER && (KIND != 3) && aF <= FMAX && !(a.ablate & 16);  // bit 16: per-wave id loads
#else
  const bool coop = !KA && !OWNER && (KIND != 3) && aF <= FMAX;
#endif
  if (coop) {
    const int64_t b0 = (int64_t)tile * 16;
    for (int t = threadIdx.x; t < 16 * aF; t += NW * 64) {
      const int ss = t / aF, c = t - ss * aF;
      const int64_t bb = b0 + ss < a.batch ? b0 + ss : a.batch - 1;
      const auto idv = I::load(a.ids, bb * a.id_stride + c);
#ifdef RS_DIAG_STAMPS
      RS_USE(idv);
      RS_STAMP(8);
#endif
      lid[ss][c] = idv;
    }
    if constexpr (!OWNER) {
      for (int t = threadIdx.x; t < 2 * aF; t += NW * 64) {
        const int c = t < aF ? t : t - aF;
        lmeta[t < aF ? 0 : 1][c] = t < aF ? a.offs[c] : a.vocab[c];
      }
    }
  }
  // ---- fields c = cg + j*NW + w; slots past F re-read field F-1 and add 0.
  // A pass = its B fragments and |v_e|^2 (launch constants), then its rows,
  // then the MFMAs.  The first two passes' B fragments are requested here,
  // inside the id trip (L2 hits, done before the ids arrive), and their norms
  // computed while the first rows are in flight, so a pass's work after its
  // rows arrive is its MFMAs and one FMA per element.
  struct Pass {
    int cj[MAXC];
    bool ok[MAXC];
    typename I::raw_t rid[MAXC];
    int64_t off[MAXC], voc[MAXC];
    int64_t row[MAXC];  // decoded table rows (decode_rows)
    Chunk<KV> xs[MAXC];
    Chunk<KV> bw[MAXC][NT];
    float nrm[MAXC][KV];
  };
  auto issue_b = [&](int cg, Pass& P) {
#pragma unroll
    for (int j = 0; j < MAXC; ++j) {
      const int c = cg + j * NW + w;
      P.cj[j] = c < aF ? c : aF - 1;
      const float* rec = a.prep + a.field_base + (int64_t)P.cj[j] * a.field_rec;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
#ifdef RS_DIAG_STAMPS
        if (a.ablate & 2) { P.bw[j][nt].zero(); P.bw[j][nt].v[0] = (float)P.cj[j]; continue; }
#endif
        // kernarg kernels: every lane loads — the packed image holds zeros in
        // its padded columns (> kfm; fm_prepare_mfma writes fm_bval's 0.f
        // there), the value the masked form puts in their place, and the exec
        // masking is code in front of the id loads.  The kernels with several
        // tiles per CU keep the mask (13.67 vs 13.61 us at B 16,384 without it).
        if (KA || nt * 16 + s <= akfm) P.bw[j][nt].load(rec + (int64_t)(nt * 64 + lane) * KV);
        else P.bw[j][nt].zero();
      }
    }
  };
  auto norms = [&](Pass& P) {
    // |v_e|^2 for this lane's element e: the B lanes of DPP row kk hold
    // v[e][0..15] — the same row as the A lane that holds x_e.
#pragma unroll
    for (int j = 0; j < MAXC; ++j)
#pragma unroll
      for (int tp = 0; tp < KV; ++tp) {
        float sq = 0.f;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const float bv = nt * 16 + s < akfm ? P.bw[j][nt].v[tp] : 0.f;
          sq = fmaf(bv, bv, sq);
        }
        P.nrm[j][tp] = row16_sum(sq);
      }
  };
  constexpr int PS = NW * MAXC;  // fields per pass
  // PF: B fragments of the first two passes ride the id trip (registers: two
  // passes only where they are few; larger rows load theirs per pass).
  // Measured (scripts/ab, profiles/r3_ab_prefetch_*.json): 14.51 vs 15.30 us
  // at batch 16384 (4 tiles per CU), 6.15 vs 6.13 at 4096 (1 tile per CU)
  constexpr bool PRE = PF && KV * MAXC * NT <= 8;
  // (the merged id load is split in the PRE block and nowhere else: the pass-at-a-time loop would decode
  // the other field's id in half the lanes and a stale id in its second pass)
  static_assert(!ID1 || PRE, "ID1 needs the two-pass schedule (PRE)");
  const int wv = threadIdx.x >> 6;
  // a pass's ids and field metadata (issue_rows takes them from here)
  auto fetch_ids = [&](int cg, Pass& P) {
    int64_t* offc = P.off;
    int64_t* vocc = P.voc;
    // Field metadata through the VECTOR path (wave index taken from the raw
    // thread id, not readfirstlane, so these are not scalar loads): issued
    // with the ids, no dependent K$-miss round trip on the critical path.
#pragma unroll
    for (int j = 0; j < MAXC; ++j) {
      if constexpr (KIND != 3) {
        if (OWNER) {
          offc[j] = 0;
          vocc[j] = a.owner_rows;
          P.rid[j] = coop ? lid[s][P.cj[j]] : I::load(a.ids, b * a.id_stride + P.cj[j]);
        } else if (coop) {
          offc[j] = lmeta[0][P.cj[j]];
          vocc[j] = lmeta[1][P.cj[j]];
          P.rid[j] = lid[s][P.cj[j]];
        } else if constexpr (KA) {  // kernarg metadata: scalar loads, wave-uniform field
          offc[j] = km->off[P.cj[j]];
          vocc[j] = km->voc[P.cj[j]];
          if constexpr (ID1) {
            // one load serves both passes of a two-pass wave: k-slots 0 / 1
            // take the first pass's field, k-slots 2 / 3 the second's (the
            // same sample, 32 lanes apart); the halves change places in front
            // of the first decode, below.  A one-pass wave loads as before.
            if (cg == 0) P.rid[j] = I::load(a.ids, b * a.id_stride + P.cj[j] + (PS + w < aF && kk >= 2 ? PS : 0));
          } else {
            P.rid[j] = I::load(a.ids, b * a.id_stride + P.cj[j]);
          }
        } else {
          const int cv = min(cg + j * NW + wv, aF - 1);
          offc[j] = a.offs[cv];
          vocc[j] = a.vocab[cv];
          P.rid[j] = I::load(a.ids, b * a.id_stride + P.cj[j]);
        }
      }
    }
    // (the two-pass schedule below requests the dense block itself, once)
    if (!PRE && cg == 0 && !coop && aF > 0) load_dense();
  };
  // id -> table row (the ids must have arrived)
  auto decode_rows = [&](int cg, Pass& P) {
    if (cg == 0) RS_STAMP(6);
    else RS_STAMP(10);
#pragma unroll
    for (int j = 0; j < MAXC; ++j) {
      if constexpr (KIND == 3) {
        P.row[j] = b * aF + P.cj[j];
        P.ok[j] = true;
      } else {
        int64_t id;
        P.ok[j] = I::decode(P.rid[j], P.voc[j], id);
        P.row[j] = P.off[j] + id;
      }
    }
    RS_USE(P.row[MAXC - 1]);
    if (cg == 0) RS_STAMP(1);
    else RS_STAMP(11);
  };
  // row gather: KV consecutive floats of the sample's row per lane
  auto load_rows = [&](int cg, Pass& P) {
#pragma unroll
    for (int j = 0; j < MAXC; ++j) {
#ifdef RS_DIAG_STAMPS
      if ((a.ablate & 8) && cg + j * NW + w >= aF) { P.xs[j].zero(); continue; }
#endif
      P.xs[j].load_nt(a.table + P.row[j] * ak + KV * kk);
    }
  };
  auto issue_rows = [&](int cg, Pass& P, bool fetched) {
    if (!fetched) fetch_ids(cg, P);
    decode_rows(cg, P);
    load_rows(cg, P);
  };
  auto consume = [&](int cg, Pass& P) {
    RS_USE(P.xs[MAXC - 1].v[KV - 1]);
    RS_USE(P.bw[MAXC - 1][0].v[KV - 1]);
    if (cg == 0) RS_STAMP(2);
    else RS_STAMP(12);
#pragma unroll
    for (int j = 0; j < MAXC; ++j) {
      const bool live = cg + j * NW + w < aF;
      if constexpr (OWNER) bad |= live && !P.ok[j] && P.rid[j] != -1;
      else bad |= live && !P.ok[j];
      const bool use = live && P.ok[j];
#pragma unroll
      for (int tp = 0; tp < KV; ++tp) {
        const float xv = use ? P.xs[j].v[tp] : 0.f;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
#ifdef RS_DIAG_STAMPS
          if (a.ablate & 1) { ac[nt][0][0] += xv * P.bw[j][nt].v[tp]; continue; }
#endif
          ac[nt][tp & 3] = mfma16x16x4(xv, P.bw[j][nt].v[tp], ac[nt][tp & 3]);
        }
        qn = fmaf(xv * xv, P.nrm[j][tp], qn);
      }
      if constexpr (TW) {
        if (live) {
          float* xo = tsm + s * xrs + P.cj[j] * ak + KV * kk;
#pragma unroll
          for (int tp = 0; tp < KV; ++tp) xo[tp] = P.ok[j] ? P.xs[j].v[tp] : 0.f;
        }
      } else if (!KA && a.x_out && live && valid) {  // (the kernarg kernel never emits x)
        float* xo = a.x_out + b * d + and_ + P.cj[j] * ak + KV * kk;
#pragma unroll
        for (int tp = 0; tp < KV; ++tp) xo[tp] = P.ok[j] ? P.xs[j].v[tp] : 0.f;
      }
    }
    RS_USE(ac[0][0][0]);
    if (cg == 0) RS_STAMP(13);
    else RS_STAMP(14);
  };
  // one slot per wave: a wave with no field left in a pass stops there (a
  // wave-uniform exit; nothing after the loop needs its slot)
  auto has_pass = [&](int cg) { return cg < aF && !(MAXC == 1 && cg + w >= aF); };
  // PL: the cold arguments' one batched s_load completes under the id trip —
  // they are first needed here, behind the B-fragment and id loads (whose
  // addresses come from preloaded SGPRs and compile-time geometry only)
  auto late_args = [&]() {
    if constexpr (PL) {
      w0v = a.w0[0];
      if constexpr (FC == 0) asm volatile("" ::"s"(a.k));
      asm volatile("" ::"s"(a.logit), "s"(a.w0), "s"(a.err));
    }
  };
  Pass P0, P1;
  // (every wave has a first field where the field count is a constant >= NW)
  const bool one = FC >= NW || has_pass(0), two = has_pass(PS);
  if (PRE) {
    if (one) issue_b(0, P0);
    if (two) issue_b(PS, P1);  // (a second field implies a first)
  }
  if (aF == 0 || coop) load_dense();
  if (coop) __syncthreads();
  RS_STAMP(9);
  if (PRE) {
    if (one) {
      // both passes' ids requested together: the second pass's id trip is
      // not serialised behind the first pass's rows and MFMAs (after the B
      // fragments: ids first was slower, 5.95 vs 5.75 us at 4096, and again
      // with the arguments preloaded, 5.94 vs 5.63)
      fetch_ids(0, P0);
      if (two) fetch_ids(PS, P1);
    }
    // the dense block, once, behind the ids (a wave with no field, F < NW,
    // may still own a dense k-step)
    if (!coop && aF > 0) load_dense();
    late_args();
    if (one) {
      if constexpr (ID1) {
        // v_permlane32_swap hands each half of the wave the other half's id:
        // every lane then holds the first pass's id in [0] and the second
        // pass's in [1] — the values the two loads put there (a one-pass wave
        // loaded its field in both halves: [0] is unchanged, [1] unused)
        if constexpr (sizeof(typename I::raw_t) == 4) {
          const auto h = __builtin_amdgcn_permlane32_swap((unsigned)P0.rid[0], (unsigned)P0.rid[0], false, false);
          P0.rid[0] = (int32_t)h[0];
          P1.rid[0] = (int32_t)h[1];
        } else {
          const uint64_t r = (uint64_t)P0.rid[0];
          const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)r, (unsigned)r, false, false);
          const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)(r >> 32), (unsigned)(r >> 32), false, false);
          P0.rid[0] = (int64_t)((uint64_t)hi[0] << 32 | lo[0]);
          P1.rid[0] = (int64_t)((uint64_t)hi[1] << 32 | lo[1]);
        }
      }
      issue_rows(0, P0, true);
      // (PL: w0, requested in late_args, is taken here, under the row trip —
      // left alone its load sinks behind the MFMAs, a dependent trip at the end)
      if constexpr (PL) asm volatile("" ::"s"(w0v));
      norms(P0);
      if (two) norms(P1);
      // the second pass's ids arrive with the first's: its row offsets are
      // worked out while the first rows are in flight and pinned in registers
      // (the empty asm), so only the loads themselves are left for later
      int64_t ro[MAXC];
#pragma unroll
      for (int j = 0; j < MAXC; ++j) ro[j] = 0;
      if (two) {
        decode_rows(PS, P1);
#pragma unroll
        for (int j = 0; j < MAXC; ++j) {
          ro[j] = P1.row[j] * ak + KV * kk;
          asm volatile("" : "+v"(ro[j]));
        }
      }
      // The second burst leaves the moment the first rows are here, and the
      // first pass's MFMAs run underneath it (both bursts at once was slower,
      // 6.19 vs 5.82 us at 4096 — the r1 finding that two row bursts beat one
      // — and the second burst behind the first pass's MFMAs left its loads
      // waiting for four waves' MFMAs on one matrix pipe: DESIGN 4.1).  Every
      // wave waits for its first rows HERE, in front of the branch: a wait
      // behind the join would be a vmcnt(0) that takes the second burst with it.
      asm volatile("" ::"v"(P0.xs[MAXC - 1].v[KV - 1]));
      __builtin_amdgcn_sched_barrier(0);
      if (two) {
#pragma unroll
        for (int j = 0; j < MAXC; ++j) {
#ifdef RS_DIAG_STAMPS
          if ((a.ablate & 8) && PS + j * NW + w >= aF) { P1.xs[j].zero(); continue; }
#endif
          P1.xs[j].load_nt(a.table + ro[j]);
        }
        RS_STAMP(15);
      }
      __builtin_amdgcn_sched_barrier(0);
      consume(0, P0);
      if (two) {
        consume(PS, P1);
        // (a third pass: more than 2 x NW fields — never in the kernarg kernel, F <= 32)
        for (int cg = 2 * PS; !KA && has_pass(cg); cg += PS) {
          issue_b(cg, P0);
          issue_rows(cg, P0, false);
          norms(P0);
          consume(cg, P0);
        }
      }
    }
  } else {
    late_args();
    // a wave with no field (F < NW, one slot per wave) may still own a dense
    // k-step: fetch_ids, which requests the dense block for the others, never
    // runs for it (without this its dense features entered as zeros)
    if (!coop && aF > 0 && !has_pass(0)) load_dense();
    for (int cg = 0; has_pass(cg); cg += PS) {
      issue_b(cg, P0);
      issue_rows(cg, P0, false);
      norms(P0);
      consume(cg, P0);
    }
  }

  // ---- dense MFMAs (their loads were issued in the prologue)
  if (has_dense) {
    const int e = 4 * dw + kk;
    dx = e < and_ ? dx : 0.f;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) ac[nt][0] = mfma16x16x4(dx, drec[nt], ac[nt][0]);
    qn = fmaf(dx * dx, dn, qn);
    if constexpr (TW) {
      if (e < and_) tsm[s * xrs + aF * ak + e] = dx;
    } else if (!KA && a.x_out && valid && e < and_) {
      a.x_out[b * d + e] = dx;
    }
  }
  if (!dense_small) {
    for (int t = w; t < a.DB; t += NW) {
      const int e = 4 * t + kk;
      const float xv = a.dense[b * a.dense_stride + (e < and_ ? e : 0)];
      const float x = e < and_ ? xv : 0.f;
      const float* rec = a.prep + (int64_t)t * a.dense_rec;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) ac[nt][0] = mfma16x16x4(x, rec[nt * 64 + lane], ac[nt][0]);
      qn = fmaf(x * x, rec[NT * 64 + kk], qn);
      if constexpr (TW) {
        if (e < and_) tsm[s * xrs + aF * ak + e] = x;
      } else if (a.x_out && valid && e < and_) {
        a.x_out[b * d + e] = x;
      }
    }
  }
  floatx4 acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[nt][i] = (ac[nt][0][i] + ac[nt][1][i]) + (ac[nt][2][i] + ac[nt][3][i]);
  RS_USE(acc[0][0]);
  RS_STAMP(3);
  if (__any(bad && valid) && lane == 0) flag_error(a.err);

#ifdef RS_DIAG_STAMPS
  if (a.ablate & 4) {
    if (w == 0 && kk == 0 && b < a.batch) a.logit[b] = acc[0][0] + acc[0][1] + qn;
    return;
  }
#endif
  // ---- combine the NW partial tiles: thread (sample, column) sums the waves'
  // partials; the per-sample reductions over columns are DPP row sums.
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int smp = kk * 4 + r, col = nt * 16 + s;
      cs[WIDE ? (smp * NC + col) * CW + w : (w * 16 + smp) * (NC + 1) + col] = acc[nt][r];
    }
  // the k-slots' q partials meet in registers: the lane swaps exchange rows
  // 16 apart, then the wave's halves, without an LDS round trip; every lane
  // adds the same two values as an xor-16 / xor-32 shuffle pair would (float
  // addition commutes), so (q0 + q1) + (q2 + q3) keeps its bits
  __builtin_amdgcn_sched_barrier(0);  // the tile writes go out first
  const auto h = __builtin_amdgcn_permlane16_swap(__float_as_uint(qn), __float_as_uint(qn), false, false);
  qn = __uint_as_float(h[0]) + __uint_as_float(h[1]);
  const auto f = __builtin_amdgcn_permlane32_swap(__float_as_uint(qn), __float_as_uint(qn), false, false);
  qn = __uint_as_float(f[0]) + __uint_as_float(f[1]);
  if (lane < 16) qs[w][lane] = qn;
  __syncthreads();
  RS_STAMP(7);
  if (threadIdx.x < 16 * NC) {
    const int smp = threadIdx.x / NC, col = threadIdx.x % NC;
    // the waves' partials in wave order 0 .. NW-1, from 0.f
    float v = 0.f;
    if constexpr (WIDE) {
      const floatx4* pw = reinterpret_cast<const floatx4*>(cs + (smp * NC + col) * CW);
      floatx4 pv[NW / 4];
#pragma unroll
      for (int g = 0; g < NW / 4; ++g) pv[g] = pw[g];
#pragma unroll
      for (int ww = 0; ww < NW; ++ww) v += pv[ww / 4][ww % 4];
    } else {
#pragma unroll
      for (int ww = 0; ww < NW; ++ww) v += cs[(ww * 16 + smp) * (NC + 1) + col];
    }
    float t = col < akfm ? v * v : 0.f;       // s_f^2
    if (col < NW) t -= qs[col][smp];           // - sum_i x_i^2 |v_i|^2 (wave partials)
    float lin = col == akfm ? v : 0.f;        // x@w1
    t = row16_sum(t);
    lin = row16_sum(lin);
    if constexpr (NT == 2) {
      t += __shfl_xor(t, 16);
      lin += __shfl_xor(lin, 16);
    }
    const int64_t bb = (int64_t)tile * 16 + smp;
    if constexpr (OWNER) {
      // partial record: column sums as they stand, the q term row-summed
      float q = col < NW ? qs[col][smp] : 0.f;
      q = row16_sum(q);
      if constexpr (NT == 2) q += __shfl_xor(q, 16);
      if (bb < a.batch) {
        float* rec = a.logit + bb * a.pstride;
        if (col <= akfm) rec[col] = v;
        if (col == 0) rec[akfm + 1] = q;
        else if (akfm + 1 + col < a.pw) rec[akfm + 1 + col] = 0.f;
      }
      return;
    }
    const float fm = (lin + w0v) + 0.5f * t;
    if (col == 0 && bb < a.batch && a.logit) a.logit[bb] = fm;
    if constexpr (TW) {
      if (col == 0) fmlog[smp] = fm;
    }
  }
  RS_STAMP(4);
  if constexpr (TW) {
    {
      const MlpArgs& a = *tw;
      MLP_STAMP(1);
    }
    mlp_tower_tile<NW>(*tw, tsm, (int64_t)tile * 16, ring, fmlog);
  }
}

// ---- the kernarg kernels with their hot arguments preloaded (RS_OPT_EMBED_FM_KERNEL 5)
// gfx950 can deliver the leading kernel arguments in user SGPRs at wave
// launch (embed_fm.hip is compiled with -amdgpu-kernarg-preload-count=14,
// _build.py), but only leading SCALAR parameters, 14 dwords at most.  So the
// seven 64-bit values the first B-fragment loads, the id loads and the first
// row addresses are made of come first, in order of first use, and the rest
// follows in a by-value struct whose s_loads complete under the id trip.
// The kernel rebuilds an EmbedFmArgs and runs the same embed_fm_body: the
// arithmetic, and so every output bit, is the struct-argument kernel's.
struct EmbedFmCold {
  float* logit;
  const float* w0;
  int* err;
  int F, k, nd, kfm;
  const int64_t* offs;
  const int64_t* vocab;
  float* x_out;
  int DB;
  int64_t dense_rec, field_rec, field_base;
  int64_t owner_rows;
  int pw;
  int64_t pstride;
  unsigned long long* dbg;
  int ablate;
};

static inline EmbedFmCold cold_args(const EmbedFmArgs& a) {
  return EmbedFmCold{a.logit, a.w0,        a.err,       a.F,          a.k,          a.nd, a.kfm,     a.offs, a.vocab,
                     a.x_out, a.DB,        a.dense_rec, a.field_rec,  a.field_base, a.owner_rows,    a.pw,   a.pstride,
                     a.dbg,   a.ablate};
}

// The packed image's geometry is a pure function of (nd, F, k, kfm): at a
// specialised shape (FC > 0) it is fm_geom's value at compile time, so the
// B-fragment addresses depend on prep and the wave index alone (the launcher
// checks it against the run-time geometry, ct_geom_matches); the generic
// instantiations take the run-time values from the cold struct.
template <int KV, int NT, int FC, int KFMC, int NDC>
__device__ __forceinline__ EmbedFmArgs hot_cold_args(const float* prep, const void* ids, int64_t id_stride,
                                                     int64_t batch, const float* dense, int64_t dense_stride,
                                                     const float* table, const EmbedFmCold& c) {
  EmbedFmArgs a;
  a.ids = ids;
  a.id_stride = id_stride;
  a.dense = dense;
  a.dense_stride = dense_stride;
  a.nd = c.nd;
  a.table = table;
  a.offs = c.offs;
  a.vocab = c.vocab;
  a.F = c.F;
  a.k = c.k;
  a.prep = prep;
  a.w0 = c.w0;
  a.kfm = c.kfm;
  a.logit = c.logit;
  a.x_out = c.x_out;
  a.batch = batch;
  a.err = c.err;
  if constexpr (FC > 0) {
    constexpr FmGeom G = fm_geom(NDC, FC, 4 * KV, KFMC);
    static_assert(G.mfma && G.KV == KV && G.NT == NT, "specialised shape: not this instantiation's geometry");
    a.DB = G.DB;
    a.dense_rec = G.dense_rec;
    a.field_rec = G.field_rec;
    a.field_base = G.field_base;
  } else {
    a.DB = c.DB;
    a.dense_rec = c.dense_rec;
    a.field_rec = c.field_rec;
    a.field_base = c.field_base;
  }
  a.owner_rows = c.owner_rows;
  a.pw = c.pw;
  a.pstride = c.pstride;
  a.dbg = c.dbg;
  a.ablate = c.ablate;
  return a;
}

}  // namespace rs
