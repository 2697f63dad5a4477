// shard_fm.hip — sharded FM, partial protocol (sharded.py).
// Owner side: rs_shard_owner_fm runs embed_fm_body in KIND 4 on the local rows
// every requester asked of this owner (pairs = requester-major samples), over
// the owner's contiguous field range; requester side: rs_shard_fm_combine sums
// the world partial records of each sample in owner order, adds the dense
// block and finishes logit = (lin + w0) + 0.5 (sum_f S_f^2 - q)
// (layer/interaction.py:106-114 regrouped; same reassociation as the headline).
// rs_shard_fm_pipe / rs_shard_fm_pipe_peer: both sides and the field route of
// a pipelined step in one launch (shard_fm_pipe).
#include <algorithm>

#include "embed_fm_body.hpp"
#include "peer.hpp"
#include "rs_common.hpp"
#include "shard_route.hpp"

namespace rs {

// ---- sharded FM, partial protocol: combine (requester side) as a block part
struct CombineArgs {
  const float* part;  // partial records [world][batch], pst floats apart
  int64_t pst;
  int world;
  int64_t batch;
  const float* dense;
  int64_t ds;
  int nd;
  const float* prep;  // the packed FM image (dense records at its start)
  int64_t dense_rec;
  int NT;
  const float* w0;
  int kfm;
  float* logit;
  // training (rs_shard_fm_combine_grad): [s_0..s_{kfm-1} | g] records gst
  // floats apart, g = (sigmoid(logit) - label) * gscale; per-sample BCE
  const float* labels;
  float gscale;
  float* gs;
  int64_t gst;
  float* loss;
};

// 16 lanes per sample (lane = partial column, strided by 16), DPP row sums;
// blocks blk of nblk, NTH threads each, grid-stride over batch*16 lanes.
template <int NTH>
__device__ __forceinline__ void fm_combine_part(const CombineArgs& c, int blk, int nblk) {
  for (int64_t idx = (int64_t)blk * NTH + threadIdx.x; idx < c.batch * 16; idx += (int64_t)nblk * NTH) {
    const int64_t b = idx >> 4;
    const int cl = threadIdx.x & 15;
    float t = 0.f, lin = 0.f, q = 0.f;
    for (int col = cl; col < c.kfm + 2; col += 16) {
      float acc = 0.f;
      for (int o = 0; o < c.world; ++o) acc += c.part[((int64_t)o * c.batch + b) * c.pst + col];
      for (int e = 0; e < c.nd; ++e) {
        const float x = c.dense[b * c.ds + e];
        const float* rec = c.prep + (int64_t)(e >> 2) * c.dense_rec;
        if (col <= c.kfm) acc = fmaf(x, rec[(col >> 4) * 64 + (e & 3) * 16 + (col & 15)], acc);
        else acc = fmaf(x * x, rec[c.NT * 64 + (e & 3)], acc);
      }
      if (col < c.kfm) {
        t = fmaf(acc, acc, t);
        if (c.gs) c.gs[b * c.gst + col] = acc;
      } else if (col == c.kfm) lin = acc;
      else q = acc;
    }
    t = row16_sum(t);
    lin = row16_sum(lin);
    q = row16_sum(q);
    if (cl == 0) {
      const float z = (lin + c.w0[0]) + 0.5f * (t - q);
      c.logit[b] = z;
      if (c.gs) {
        const float y = c.labels[b];
        c.gs[b * c.gst + c.kfm] = (sigmoidf_(z) - y) * c.gscale;
        if (c.loss) c.loss[b] = fmaxf(z, 0.f) - z * y + log1pf(expf(-fabsf(z)));
      }
    }
  }
}

// One launch per pipelined step (sharded.py pipe_step): blocks
// [0, owner_blocks) are the owner side of batch t (KIND 4, 16 pairs each),
// then route_blocks of batch t+1's field route, then combine_blocks of batch
// t-1's combine — three independent parts, so a step is ONE kernel + ONE
// all-to-all.  Any part may be empty.
struct PipeArgs {
  int owner_blocks, route_blocks, combine_blocks;
  RouteArgs r;
  CombineArgs c;
  // two-deep peer step (rs_shard_fm_pipe_peer, XCHG): the exchange of the
  // NEXT batch's records (x.chunks x x.world workgroups, first in dispatch
  // order) rides in this launch beside the pipe parts of this batch
  int xchg_blocks;
  PeerArgs x;
};

template <int KV, int NT, int NW, int MC, bool XCHG = false, int FC = 0, int KFMC = 0>
__global__ __launch_bounds__(NW * 64) void shard_fm_pipe(EmbedFmArgs a, PipeArgs p) {
  // the short route / combine blocks come first in dispatch order, the owner
  // blocks (the headline kernel's body) after them: dispatched last, the
  // owner tiles spread over the CUs the short blocks leave instead of
  // doubling up behind them.  XCHG: the exchange workgroups before all of
  // them (workgroup 0 publishes this rank's mailbox readiness at once; they
  // wait on peers, never on the other parts of this launch, and those never
  // wait, so the launch drains whatever the dispatch order)
  int bid = blockIdx.x;
  if constexpr (XCHG) {
    if (bid < p.xchg_blocks) {
      peer_a2a_part<false>(p.x, bid / p.x.world, bid % p.x.world);
      return;
    }
    bid -= p.xchg_blocks;
  }
  if (bid < p.route_blocks) {
    field_route_part<NW * 64>(p.r, bid, p.route_blocks);
  } else if (bid < p.route_blocks + p.combine_blocks) {
    fm_combine_part<NW * 64>(p.c, bid - p.route_blocks, p.combine_blocks);
  } else {
    // the headline kernel's schedule: B fragments of the first two passes and
    // both passes' ids issued before the first rows (PF)
    embed_fm_body<KV, NT, NW, 4, false, MC, true, false, FC, KFMC, (FC > 0 ? 0 : -1)>(
        a, nullptr, bid - p.route_blocks - p.combine_blocks);
  }
}

template <int KV, int NT, int NW, int MC, bool XCHG = false>
static void launch_pipe4(const EmbedFmArgs& a, PipeArgs p, hipStream_t st) {
  const int T = NW * 64;
  p.owner_blocks = a.F > 0 ? (int)((a.batch + 15) / 16) : 0;
  if (p.route_blocks) p.route_blocks = (int)std::min<int64_t>((p.r.total + T - 1) / T, 4096);
  if (p.combine_blocks) p.combine_blocks = (int)std::min<int64_t>((p.c.batch * 16 + T - 1) / T, 4096);
  if (!XCHG) p.xchg_blocks = 0;
  const int grid = p.xchg_blocks + p.owner_blocks + p.route_blocks + p.combine_blocks;
  if (!grid) return;
  if constexpr (KV == 4 && NT == 1 && NW == 16 && MC == 1) {
    // the world-1 owner of the Criteo table (all 26 fields, kfm 10, no dense
    // block): field count and FM width as constants (as the headline kernel)
    if (a.F == 26 && a.kfm == 10 && a.nd == 0) {
      shard_fm_pipe<KV, NT, NW, MC, XCHG, 26, 10><<<grid, T, 0, st>>>(a, p);
      return;
    }
  }
  shard_fm_pipe<KV, NT, NW, MC, XCHG><<<grid, T, 0, st>>>(a, p);
}

// the two-deep peer step: 1-tile (kfm <= 15) owner part with <= 32 fields
template <int KV>
static void launch_pipe_xchg_kv(const EmbedFmArgs& a, const PipeArgs& p, hipStream_t st) {
  if (a.F <= 4) launch_pipe4<KV, 1, 4, 1, true>(a, p, st);
  else if (a.F <= 8) launch_pipe4<KV, 1, 8, 1, true>(a, p, st);
  else launch_pipe4<KV, 1, 16, 1, true>(a, p, st);
}
static void launch_pipe_xchg(const EmbedFmArgs& a, const PipeArgs& p, const FmGeom& g, hipStream_t st) {
  with_kv(g.KV, [&](auto kv) { launch_pipe_xchg_kv<decltype(kv)::value>(a, p, st); });
}

// NW / MC by the owner's field count: 4 waves x 1 slot for <= 4 fields (the
// 8-rank shape), 8 waves for <= 8 (4 ranks), 16 waves x 1 slot per pass up
// to 32 fields (as the headline kernel), 2 slots per pass beyond.
template <int KV>
static void launch_pipe_kv(const EmbedFmArgs& a, const PipeArgs& p, int NT, hipStream_t st) {
  if (NT == 1 && a.F <= 4) launch_pipe4<KV, 1, 4, 1>(a, p, st);
  else if (NT == 1 && a.F <= 8) launch_pipe4<KV, 1, 8, 1>(a, p, st);
  else if (NT == 1 && a.F <= 32) launch_pipe4<KV, 1, 16, 1>(a, p, st);
  else if (NT == 1) launch_pipe4<KV, 1, 16, 0>(a, p, st);
  else if (a.F <= 32) launch_pipe4<KV, 2, 16, 1>(a, p, st);
  else launch_pipe4<KV, 2, 16, 0>(a, p, st);
}

static void launch_pipe(const EmbedFmArgs& a, const PipeArgs& p, const FmGeom& g, hipStream_t st) {
  with_kv(g.KV, [&](auto kv) { launch_pipe_kv<decltype(kv)::value>(a, p, g.NT, st); });
}

// owner part (KIND 4) of a pipe launch over the received row-id records
static EmbedFmArgs owner_args(const FmGeom& g, const int32_t* local_rows, int64_t rec_stride, int field_lo,
                              int n_owned, const float* shard, int64_t shard_rows, int k, const float* prepared,
                              int kfm, float* partial, int64_t partial_stride, int64_t n_pairs, int* err_flag) {
  // (no dense block, no field metadata, no w0; prep: the weights of the owner's first field)
  EmbedFmArgs a = fm_args(local_rows, rec_stride, nullptr, 0, 0, shard, nullptr, nullptr, n_owned, k,
                          prepared + (int64_t)field_lo * g.field_rec, nullptr, kfm, partial, nullptr, n_pairs, err_flag);
  set_geom(a, g);
  a.DB = 0;  // dense block: added by the requester (combine part)
  a.owner_rows = shard_rows;
  a.pw = (kfm + 2 + 3) / 4 * 4;
  a.pstride = partial_stride;
  return a;
}

}  // namespace rs

using namespace rs;

extern "C" int rs_fm_partial_width(int kfm) { return kfm < 1 ? -1 : (kfm + 2 + 3) / 4 * 4; }

#define RS_PIPE_GEOM(what)                                                                  \
  const FmGeom g = fm_geom(nd, n_fields, k, kfm);                                            \
  if (!g.mfma) {                                                                             \
    set_error("%s: needs the packed FM image (k in {4,8,16,32,64}, kfm <= 31)", what);       \
    return RS_ERR_UNSUPPORTED;                                                               \
  }                                                                                          \
  const int pw = (kfm + 2 + 3) / 4 * 4;                                                      \
  (void)pw

extern "C" int rs_shard_owner_fm(const int32_t* local_rows, int64_t rec_stride, int field_lo, int n_owned,
                                 const float* shard, int64_t shard_rows, int nd, int n_fields, int k,
                                 const float* prepared, int kfm, float* partial, int64_t partial_stride,
                                 int64_t n_pairs, int* err_flag, rs_stream_t stream) {
  if (n_pairs == 0) return RS_OK;  // empty batch: nothing to launch
  RS_REQUIRE(n_pairs > 0 && kfm >= 1 && nd >= 0 && k >= 1 && field_lo >= 0 && n_owned >= 0 &&
                 field_lo + n_owned <= n_fields && n_owned <= rec_stride && shard_rows >= 0,
             "rs_shard_owner_fm: bad shape");
  RS_REQUIRE(prepared && partial && (n_owned == 0 || (local_rows && (shard || shard_rows == 0))),
             "rs_shard_owner_fm: null pointer");
  RS_REQUIRE((uintptr_t)shard % 16 == 0, "rs_shard_owner_fm: shard must be 16-B aligned");
  RS_PIPE_GEOM("rs_shard_owner_fm");
  RS_REQUIRE(partial_stride >= pw, "rs_shard_owner_fm: partial_stride < rs_fm_partial_width");
  hipStream_t st = as_stream(stream);
  if (n_owned == 0) {  // this owner holds no rows: every partial is zero
    (void)hipMemset2DAsync(partial, partial_stride * sizeof(float), 0, pw * sizeof(float), n_pairs, st);
    return launch_status("rs_shard_owner_fm");
  }
  PipeArgs p{};
  launch_pipe(owner_args(g, local_rows, rec_stride, field_lo, n_owned, shard, shard_rows, k, prepared, kfm, partial,
                         partial_stride, n_pairs, err_flag),
              p, g, st);
  return launch_status("rs_shard_owner_fm");
}

extern "C" int rs_shard_fm_combine(const float* partials, int64_t partial_stride, int world, int64_t batch,
                                   const float* dense, int64_t dense_stride, int nd, int n_fields, int k,
                                   const float* prepared, const float* w0, int kfm, float* logit,
                                   rs_stream_t stream) {
  if (batch == 0) return RS_OK;  // empty batch: nothing to launch
  RS_REQUIRE(batch > 0 && world >= 1 && nd >= 0 && n_fields >= 0 && kfm >= 1, "rs_shard_fm_combine: bad shape");
  RS_REQUIRE(partials && prepared && w0 && logit && (nd == 0 || dense), "rs_shard_fm_combine: null pointer");
  RS_PIPE_GEOM("rs_shard_fm_combine");
  RS_REQUIRE(partial_stride >= pw, "rs_shard_fm_combine: partial_stride < rs_fm_partial_width");
  EmbedFmArgs a{};  // no owner part
  PipeArgs p{};
  p.combine_blocks = 1;
  p.c = CombineArgs{partials, partial_stride, world, batch, dense, dense_stride, nd, prepared, g.dense_rec, g.NT,
                    w0, kfm, logit};
  launch_pipe(a, p, g, as_stream(stream));
  return launch_status("rs_shard_fm_combine");
}

extern "C" int rs_shard_fm_combine_grad(const float* partials, int64_t partial_stride, int world, int64_t batch,
                                        const float* dense, int64_t dense_stride, int nd, int n_fields, int k,
                                        const float* prepared, const float* w0, int kfm, const float* labels,
                                        float grad_scale, float* logit, float* gs, int64_t gs_stride, float* loss,
                                        rs_stream_t stream) {
  if (batch == 0) return RS_OK;
  RS_REQUIRE(batch > 0 && world >= 1 && nd >= 0 && n_fields >= 0 && kfm >= 1 && gs_stride >= kfm + 1,
             "rs_shard_fm_combine_grad: bad shape");
  RS_REQUIRE(partials && prepared && w0 && logit && labels && gs && (nd == 0 || dense),
             "rs_shard_fm_combine_grad: null pointer");
  RS_PIPE_GEOM("rs_shard_fm_combine_grad");
  RS_REQUIRE(partial_stride >= pw, "rs_shard_fm_combine_grad: partial_stride < rs_fm_partial_width");
  EmbedFmArgs a{};
  PipeArgs p{};
  p.combine_blocks = 1;
  p.c = CombineArgs{partials, partial_stride, world, batch, dense, dense_stride, nd, prepared, g.dense_rec, g.NT,
                    w0, kfm, logit, labels, grad_scale, gs, gs_stride, loss};
  launch_pipe(a, p, g, as_stream(stream));
  return launch_status("rs_shard_fm_combine_grad");
}

// What rs_shard_fm_pipe and rs_shard_fm_pipe_peer share (`what`: the entry
// point's name; own_shape_ok: its own conditions on the shape): the argument
// checks, then the parts of the launch — the owner part over the received
// records (this rank owns no rows: its partials zeroed for every requester
// instead), the route of the next batch, the combine of the previous one.
struct PipeStep {
  FmGeom g;
  EmbedFmArgs a;
  PipeArgs p;
  int64_t R;  // words per fused record: [row ids | partial]
};
static int pipe_step(const char* what, bool own_shape_ok, const int32_t* recv, int32_t* send, int field_lo,
                     int n_owned, const float* shard, int64_t shard_rows, const float* dense_prev,
                     int64_t dense_stride, float* logit_prev, const void* ids_next, int id_kind, int64_t id_stride,
                     const int64_t* field_offsets, const int64_t* field_vocab, int64_t rows_per_rank,
                     const int32_t* owner_fields, int slot_stride, int world, int64_t batch, int nd, int n_fields,
                     int k, const float* prepared, const float* w0, int kfm, int* err_flag, hipStream_t st,
                     PipeStep& s) {
  RS_REQUIRE(own_shape_ok && batch > 0 && world >= 1 && nd >= 0 && n_fields >= 1 && k >= 1 && kfm >= 1 &&
                 slot_stride >= 1 && slot_stride <= n_fields && field_lo >= 0 && n_owned >= 0 &&
                 field_lo + n_owned <= n_fields && n_owned <= slot_stride && shard_rows >= 0 && rows_per_rank >= 1,
             "%s: bad shape", what);
  RS_REQUIRE(recv && send && prepared && w0 && (n_owned == 0 || shard || shard_rows == 0), "%s: null pointer", what);
  RS_REQUIRE(!ids_next || (field_offsets && field_vocab && owner_fields), "%s: route inputs missing", what);
  RS_REQUIRE(!logit_prev || nd == 0 || dense_prev, "%s: dense_prev is null", what);
  RS_REQUIRE((uintptr_t)shard % 16 == 0, "%s: shard must be 16-B aligned", what);
  RS_REQUIRE((int64_t)world * batch * (slot_stride + 32) < ((int64_t)1 << 31) && rows_per_rank < ((int64_t)1 << 31),
             "%s: too many slots / shard rows must fit int32", what);
  RS_REQUIRE(id_kind >= RS_ID_I32 && id_kind <= RS_ID_F32, "%s: bad id_kind", what);
  RS_PIPE_GEOM(what);
  const int64_t R = slot_stride + pw;
  const int64_t n_pairs = (int64_t)world * batch;
  float* pout = reinterpret_cast<float*>(send + slot_stride);
  const float* pin = reinterpret_cast<const float*>(recv + slot_stride);
  s = PipeStep{g, EmbedFmArgs{}, PipeArgs{}, R};
  if (n_owned > 0) {
    s.a = owner_args(g, recv, R, field_lo, n_owned, shard, shard_rows, k, prepared, kfm, pout, R, n_pairs, err_flag);
  } else {
    (void)hipMemset2DAsync(pout, R * sizeof(float), 0, pw * sizeof(float), n_pairs, st);
  }
  if (ids_next) {
    s.p.route_blocks = 1;
    s.p.r = RouteArgs{ids_next, id_kind, id_stride, field_offsets, field_vocab, rows_per_rank, owner_fields,
                      slot_stride, (int)batch, R, send, err_flag, (int64_t)world * batch * slot_stride};
  }
  if (logit_prev) {
    s.p.combine_blocks = 1;
    s.p.c = CombineArgs{pin, R, world, batch, dense_prev, dense_stride, nd, prepared, g.dense_rec, g.NT, w0, kfm,
                        logit_prev};
  }
  return RS_OK;
}

extern "C" int rs_shard_fm_pipe(const int32_t* recv, int field_lo, int n_owned, const float* shard,
                                int64_t shard_rows, const float* dense_prev, int64_t dense_stride, float* logit_prev,
                                const void* ids_next, int id_kind, int64_t id_stride, const int64_t* field_offsets,
                                const int64_t* field_vocab, int64_t rows_per_rank, const int32_t* owner_fields,
                                int slot_stride, int32_t* send, int world, int64_t batch, int nd, int n_fields,
                                int k, const float* prepared, const float* w0, int kfm, int* err_flag,
                                rs_stream_t stream) {
  if (batch == 0) return RS_OK;  // empty batch: nothing to launch
  hipStream_t st = as_stream(stream);
  PipeStep s;
  if (const int rc = pipe_step("rs_shard_fm_pipe", world <= 64, recv, send, field_lo, n_owned, shard, shard_rows,
                               dense_prev, dense_stride, logit_prev, ids_next, id_kind, id_stride, field_offsets,
                               field_vocab, rows_per_rank, owner_fields, slot_stride, world, batch, nd, n_fields, k,
                               prepared, w0, kfm, err_flag, st, s))
    return rc;
  launch_pipe(s.a, s.p, s.g, st);
  return launch_status("rs_shard_fm_pipe");
}

// The two-deep pipelined step with the peer exchange inside the launch:
// launch t = exchange of batch t+1's records [row ids of t+1 | partials of
// t-1] (send slot xslot -> every peer's mailbox slot xslot) | combine of t-2 |
// owner partials of t | route of t+2, the pipe parts reading this rank's
// mailbox slot (recv) and writing send slot t % 2 (send).  Host contract in
// sharded.py (ShardedEmbeddingFM.pipe2_step); protocol in peer.hip.
extern "C" int rs_shard_fm_pipe_peer(const int32_t* recv, int32_t* send, const int32_t* xsend, int xslot,
                                     int exchange, int field_lo, int n_owned, const float* shard, int64_t shard_rows,
                                     const float* dense_prev, int64_t dense_stride, float* logit_prev,
                                     const void* ids_next, int id_kind, int64_t id_stride,
                                     const int64_t* field_offsets, const int64_t* field_vocab, int64_t rows_per_rank,
                                     const int32_t* owner_fields, int slot_stride, int world, int64_t batch, int nd,
                                     int n_fields, int k, const float* prepared, const float* w0, int kfm,
                                     int* err_flag, void* const* mailboxes, int rank, void* peer_state, int chunks,
                                     int64_t spin_limit, int* xerr, rs_stream_t stream) {
  if (batch == 0) return RS_OK;
  RS_REQUIRE(!exchange || (xsend && mailboxes && peer_state && xerr), "rs_shard_fm_pipe_peer: exchange inputs missing");
  RS_REQUIRE(!exchange || (chunks >= 1 && (int64_t)chunks * world <= 1024 && spin_limit >= 1),
             "rs_shard_fm_pipe_peer: bad chunks / limit");
  // the 1-tile owner part with <= 32 fields only (launch_pipe_xchg_kv)
  if (fm_geom(nd, n_fields, k, kfm).NT > 1 || n_owned > 32) {
    set_error("rs_shard_fm_pipe_peer: needs kfm <= 15 and <= 32 owned fields");
    return RS_ERR_UNSUPPORTED;
  }
  hipStream_t st = as_stream(stream);
  PipeStep s;
  if (const int rc = pipe_step("rs_shard_fm_pipe_peer",
                               world <= PEER_MAXW && rank >= 0 && rank < world && (xslot == 0 || xslot == 1), recv,
                               send, field_lo, n_owned, shard, shard_rows, dense_prev, dense_stride, logit_prev,
                               ids_next, id_kind, id_stride, field_offsets, field_vocab, rows_per_rank, owner_fields,
                               slot_stride, world, batch, nd, n_fields, k, prepared, w0, kfm, err_flag, st, s))
    return rc;
  PipeArgs& p = s.p;
  if (exchange) {
    const int64_t blk = batch * s.R * 4;  // bytes of one rank's records for one peer
    if (blk % 16) {
      set_error("rs_shard_fm_pipe_peer: batch * record bytes must be a multiple of 16");
      return RS_ERR_ARG;
    }
    p.xchg_blocks = chunks * world;
    p.x = PeerArgs{reinterpret_cast<const char*>(xsend), blk, reinterpret_cast<char* const*>(mailboxes),
                   (2 * (int64_t)world * blk + 255) / 256 * 256, static_cast<PeerState*>(peer_state), rank, world,
                   chunks, spin_limit, xerr, nullptr, 0, nullptr, 0, (int64_t)xslot * world * blk,
                   opt(RS_OPT_PEER_FENCES) == 0};
  }
  launch_pipe_xchg(s.a, p, s.g, st);
  return launch_status("rs_shard_fm_pipe_peer");
}
