// embed_fm.hpp — shared declarations of the fused gather + FM kernels
// (embed_fm.hip: MFMA K-split kernel; shard_fm.hip: sharded owner / pipe
// parts; deepfm.hip: fused DeepFM; embed_gather.hip: plain gather and one-hot
// FM; embed_fm_tiles.hip: the pipelined MFMA and VALU/DPP kernels of
// rs_embed_fm_fwd) and the host helpers that fill their launch arguments.
// Reference: FMLayer.call, layer/interaction.py:106-114.
#pragma once
#include "rs_common.hpp"

namespace rs {

// ----------------------------------------------------------- packed layout
struct FmGeom {
  int nd, F, k, kfm, d;
  bool mfma;
  int KV, NT, DB;
  int64_t dense_rec, field_rec, field_base, size;
};

// (constexpr: the kernels specialised for one shape take it at compile time)
static inline constexpr FmGeom fm_geom(int nd, int F, int k, int kfm) {
  FmGeom g{};
  g.nd = nd;
  g.F = F;
  g.k = k;
  g.kfm = kfm;
  g.d = nd + F * k;
  const bool kv_ok = (F == 0) || (k % 4 == 0 && (k == 4 || k == 8 || k == 16 || k == 32 || k == 64));
  g.mfma = kv_ok && kfm >= 1 && kfm + 1 <= 32;
  if (g.mfma) {
    g.KV = (F == 0) ? 4 : k / 4;
    g.NT = (kfm + 1 + 15) / 16;
    g.DB = (nd + 3) / 4;
    g.dense_rec = (int64_t)g.NT * 64 + 4;
    g.field_rec = (int64_t)g.NT * 64 * g.KV + 4 * g.KV;
    g.field_base = (int64_t)g.DB * g.dense_rec;
    g.size = g.field_base + (int64_t)F * g.field_rec;
  } else {
    // generic path: [w1 (d) | v (d*kfm) | |v_i|^2 (d)]
    g.size = (int64_t)g.d * (kfm + 2);
  }
  return g;
}

// ----------------------------------------------------------- arguments
struct EmbedFmArgs {
  const void* ids;
  int64_t id_stride;
  const float* dense;
  int64_t dense_stride;
  int nd;
  const float* table;
  const int64_t* offs;
  const int64_t* vocab;
  int F;
  int k;
  const float* prep;
  const float* w0;
  int kfm;
  float* logit;
  float* x_out;
  int64_t batch;
  int* err;
  int DB;
  int64_t dense_rec, field_rec, field_base;
  int64_t owner_rows;       // KIND 4: rows of the owner's shard (ids are local rows, -1 = absent)
  int pw;                   // KIND 4: floats per partial record (logit -> partial records)
  int64_t pstride;          // KIND 4: floats between consecutive samples' partial records
  unsigned long long* dbg;  // diagnostic builds only (RS_DIAG_STAMPS): phase stamps
  int ablate;               // diagnostic builds only: bit0 no MFMA, bit1 no B loads, bit2 no combine
};

// Field metadata by value in the kernarg (diagnostic build -DRS_DIAG_KARG:
// the per-wave id path reads it through scalar loads, no LDS id tile)
struct FieldMeta {
  int64_t off[32];
  int64_t voc[32];
};

// ----------------------------------------------------------- host helpers
// The entry points' arguments as an EmbedFmArgs (everything else zero; the
// packed image's geometry: set_geom).
static inline EmbedFmArgs fm_args(const void* ids, int64_t id_stride, const float* dense, int64_t dense_stride, int nd,
                                  const float* table, const int64_t* offs, const int64_t* vocab, int F, int k,
                                  const float* prep, const float* w0, int kfm, float* logit, float* x_out,
                                  int64_t batch, int* err) {
  EmbedFmArgs a{};
  a.ids = ids;
  a.id_stride = id_stride;
  a.dense = dense;
  a.dense_stride = dense_stride;
  a.nd = nd;
  a.table = table;
  a.offs = offs;
  a.vocab = vocab;
  a.F = F;
  a.k = k;
  a.prep = prep;
  a.w0 = w0;
  a.kfm = kfm;
  a.logit = logit;
  a.x_out = x_out;
  a.batch = batch;
  a.err = err;
  return a;
}

static inline void set_geom(EmbedFmArgs& a, const FmGeom& g) {
  a.DB = g.DB;
  a.dense_rec = g.dense_rec;
  a.field_rec = g.field_rec;
  a.field_base = g.field_base;
}

// the first n (<= 32) fields' host-side (offset, vocab) pairs by value
static inline FieldMeta field_meta(const int64_t* host_offs, const int64_t* host_vocab, int n) {
  FieldMeta m{};
  for (int c = 0; c < n; ++c) {
    m.off[c] = host_offs[c];
    m.voc[c] = host_vocab[c];
  }
  return m;
}

// the same into m for the kernarg front ends of the cross and product
// families (k = 16, 1..32 fields, both host arrays given), else null
static inline const FieldMeta* kernarg_meta(FieldMeta& m, const int64_t* host_offs, const int64_t* host_vocab, int n,
                                            int k) {
  if (!host_offs || !host_vocab || k != 16 || n < 1 || n > 32) return nullptr;
  m = field_meta(host_offs, host_vocab, n);
  return &m;
}

static inline int grid_for(int64_t work, int block, int cap = 2048) {
  int64_t g = (work + block - 1) / block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (int)g;
}

// Launches of embed_fm_tiles.hip (rs_embed_fm_fwd, id kinds 0..2): returns
// false when the shape / option has no kernel there (the caller then runs the
// K-split kernel of embed_fm.hip).
bool launch_embed_fm_tiles(const EmbedFmArgs& a, const FmGeom& g, int kind, int variant, hipStream_t st);

}  // namespace rs
