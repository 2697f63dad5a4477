/*
 * rs_capi.h — C-ABI of the MI355X-native CTR forward path (librs_hip.so).
 *
 * This is the drop-in boundary that replaces the TF/Keras ops used by the
 * reference's embedding-lookup + feature-interaction forward path
 * (Hcyand/recommender_system, algorithm/deep_learning/...).  Every entry point
 * below cites the reference interface it replaces.  The Python host layer
 * (recommender_system_amd/layers.py, models.py) mirrors the reference's Keras
 * Layer/Model API on top of these functions; any other host (ctypes, cgo, JNI)
 * binds the same symbols.
 *
 * Conventions
 *  - All tensors are caller-owned DEVICE pointers (HBM), row-major, contiguous
 *    unless a *_stride argument says otherwise (strides are in ELEMENTS).
 *  - Sizes are int64_t; small shape parameters are int.
 *  - Every function is stream-ordered on `stream` (a hipStream_t passed as
 *    void*; NULL = the legacy default stream), never allocates, never
 *    synchronises, and is safe to capture into a hipGraph.
 *  - Return value: RS_OK (0) or a negative rs_status; the message for the last
 *    failure on the calling thread is available from rs_last_error_string().
 *  - Sparse ids: `id_kind` selects int32 / int64 / float32.  float32 ids follow
 *    the reference's packed input X[B,39] (model/deepFM.py:24), where Keras'
 *    Embedding casts float ids to int32 by truncation.  An id outside
 *    [0, vocab_c) is an error in the reference (TF InvalidArgumentError on CPU);
 *    here the kernel reads a zero row instead and sets *err_flag = 1 (if
 *    err_flag != NULL), which the host layer turns into IndexError.
 */
#ifndef RS_CAPI_H
#define RS_CAPI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* rs_stream_t; /* hipStream_t */

enum rs_status {
  RS_OK = 0,
  RS_ERR_ARG = -1,         /* bad shape / null pointer / unsupported combination */
  RS_ERR_HIP = -2,         /* HIP launch or runtime error */
  RS_ERR_UNSUPPORTED = -3  /* valid request, no kernel for it in this build */
};

enum rs_id_kind { RS_ID_I32 = 0, RS_ID_I64 = 1, RS_ID_F32 = 2 };

enum rs_act {
  RS_ACT_NONE = 0,
  RS_ACT_RELU = 1,
  RS_ACT_PRELU = 2,   /* max(0,x) + alpha*min(0,x); alpha per output column  */
  RS_ACT_SIGMOID = 3
};

/* Bits of the device error flag (int, caller-owned, zero it before use):
 * kernels OR these in; the host layer raises IndexError for RS_FLAG_BAD_ID
 * (TF's InvalidArgumentError on an out-of-range Embedding id; its BadIdError
 * is an IndexError and an RSError) and a plain RSError for any other bit. */
enum rs_flag {
  RS_FLAG_BAD_ID = 1, /* an id outside [0, vocab) (its row read as zeros)               */
  RS_FLAG_LAYOUT = 2, /* field row ranges overlap or decrease where a kernel needs the
                         concatenated-table layout (offset_c + vocab_c <= offset_{c+1}) */
  RS_FLAG_TIMEOUT = 4 /* a bounded in-kernel wait (a workgroup-internal hand-off) gave up:
                         a kernel logic error — the launch's outputs are invalid and the
                         host layer raises RSError instead of returning them               */
};

/* Runtime tuning options (host side, read when a kernel is launched, so a
 * captured hipGraph keeps the value it was captured with).  Options are
 * THREAD-LOCAL: rs_set_option changes only the launches made by the calling
 * host thread, every new thread starts from the defaults — no process-wide
 * mutable state, so concurrent callers on different threads stay reentrant
 * (SURVEY 8(b)).  They select between measured kernel forms for A/B work;
 * results agree within the parity tolerance whatever the setting. */
enum rs_option {
  RS_OPT_EMBED_FM_KERNEL = 0, /* rs_embed_fm_fwd kernel (id inputs, no x_out): 0 = MFMA K-split,
                                 1 = VALU/DPP persistent 8-sample tiles, 2 / 3 = MFMA persistent
                                 16-sample tiles (2 / 1 resident per CU); shapes a kernel does
                                 not cover run the K-split one.  4 / 5 = the K-split kernel, and
                                 on the host-metadata entries (rs_embed_fm_fwd_hm, _hm_stream) its
                                 kernarg form: 4 = all arguments in one by-value struct, 5 = the
                                 hot arguments first, preloaded into SGPRs (0 takes the measured
                                 default of the two; bit-identical).  See DESIGN.md 4.1           */
  RS_OPT_MLP_UNROLL = 1,      /* fused MLP towers (rs_mlp_fwd, rs_deepfm_fwd, rs_dcn_fwd): 1 (the
                                 default) = the k-group loop of the common layer widths fully
                                 unrolled (no loop-head wait on the weight ring), 0 = the looped
                                 form.  See DESIGN.md 4.5                                         */
  RS_OPT_DEEPFM_KERNEL = 2,   /* rs_deepfm_fwd_hm at the Criteo shape (k 16, 26 fields, 256-unit
                                 first layer): 0 (the default) = split wave roles (loaders +
                                 layer-0 compute waves, deepfm_ws), 1 = one role per wave (gather
                                 + FM, then the tower), 2 / 3 = every wave gathers two fields and
                                 computes one layer-0 tile, split-K tower tail (deepfm_all; a
                                 weight ring 3 / 4 k-groups deep).  See DESIGN.md 4.5            */
  RS_OPT_DIN_KERNEL = 3,      /* rs_din_attention_ids_fwd at the reference's (80, 40) widths: 0
                                 (the default) = one launch (scores + softmax + pool, din_fused),
                                 1 = two launches (din_scores, din_pool).  See DESIGN.md 4.4     */
  RS_OPT_PEER_FENCES = 4,     /* the peer-mapped exchange's ordering (rs_peer_a2a, rs_peer_gather_a2a,
                                 rs_shard_fm_pipe_peer): 0 (the default) = lean — write-through
                                 data stores, relaxed counts, write-through flags, no L2
                                 maintenance; 1 = a system-scope release / acquire fence around
                                 every count and flag.  See DESIGN.md 4.6                        */
  RS_OPT_CROSS_KERNEL = 5,    /* rs_embed_cross_fwd_hm / rs_dcn_fwd_hm (k 16, <= 32 fields, <= 16
                                 CrossNet B columns): 0
                                 (the default) = the contraction from the gathered registers as
                                 the rows land; 1 = the staged-tile contraction after the gather
                                 (bit-identical to rs_embed_cross_fwd).  See DESIGN.md 4.2       */
  RS_OPT_COUNT = 6
};

/* ------------------------------------------- peer-mapped exchange (§8(e))
 * An equal-split all-to-all for the sharded lookup's fixed-size record
 * exchanges without RCCL (csrc/peer.hip, sharded.py PeerExchange): every rank
 * owns one mailbox (rs_peer_alloc: uncached device memory, zeroed) of
 * rs_peer_mailbox_bytes(world, block_bytes) bytes = [world][block_bytes] data
 * + step flags, exports it (rs_peer_ipc_handle: a 64-byte hipIpcMemHandle_t)
 * and maps every peer's (rs_peer_ipc_open).  rs_peer_a2a is ONE launch per
 * exchange: rank `rank` writes block p of `send` into rank p's mailbox at
 * data[rank] once p has flagged its mailbox free for the step, flags it, and
 * the launch ends when every rank's block of the step is in its own mailbox.
 * mailboxes: device array [world] of every rank's mailbox base as seen by
 * this process (its own at [rank]); state: rs_peer_state_bytes() of zeroed
 * device memory, private to this rank and exchange (the step counter lives
 * there: graph-capturable).  Kernels that read the received data must run on
 * `stream` after the call and before the next rs_peer_a2a of the same
 * mailbox.  Bounded waits (spin_limit polls): a timeout sets RS_FLAG_TIMEOUT
 * in *err_flag.  block_bytes % 16 == 0, world <= 64, chunks * world <= 1024.
 * No reference counterpart (the reference has no distributed code).     */
int64_t rs_peer_state_bytes(void);
int64_t rs_peer_mailbox_bytes(int world, int64_t block_bytes);
int rs_peer_alloc(int64_t bytes, void** ptr);
int rs_peer_free(void* ptr);
int rs_peer_ipc_handle(void* ptr, void* handle64);
int rs_peer_ipc_open(const void* handle64, void** ptr);
int rs_peer_ipc_close(void* ptr);
int rs_peer_a2a(const void* send, int64_t block_bytes, void* const* mailboxes,
                int rank, int world, void* state, int chunks,
                int64_t spin_limit, int* err_flag, rs_stream_t stream);
/* The owner's row service fused with the row exchange (config 5): block p
 * for rank p is gathered on the fly — for every word i of ids[p][0..nw) the
 * 64-B row table[ids[p][i]] of the local shard (k = 16; -1 = a zero row, any
 * other id outside [0, n_rows) a zero row + RS_FLAG_BAD_ID) — and written
 * straight into rank p's mailbox (block_bytes = nw * 64); the same flags,
 * waits and state as rs_peer_a2a.  Replaces rs_gather_rows + the row
 * all-to-all of sharded.py ShardedDeepFM.                                 */
int rs_peer_gather_a2a(const int32_t* ids, int64_t nw, const float* table,
                       int64_t n_rows, int k, void* const* mailboxes, int rank,
                       int world, void* state, int chunks, int64_t spin_limit,
                       int* err_flag, rs_stream_t stream);

/* ------------------------------------------------------------------ meta */
const char* rs_version(void);
const char* rs_last_error_string(void);
/* Set option `option` to `value`; returns the previous value, or -1 for an
 * unknown option / out-of-range value (then nothing changes). */
int rs_set_option(int option, int value);
/* Current value of `option`, or -1 for an unknown option. */
int rs_get_option(int option);
/* Diagnostic (no reference counterpart): launch an empty kernel of `grid`
 * workgroups x `block` threads on `stream`.  bench.py replays it from a
 * hipGraph to record the box's dependent-launch slot time beside its
 * numbers. */
int rs_diag_empty(int grid, int block, rs_stream_t stream);
/* rs_diag_wave_slots: every wave's HW_ID register (bits 3:0 wave slot, 5:4
 * SIMD, 11:8 CU, 12 SH, 15:13 SE) into out[grid * block / 64], lds_bytes of
 * dynamic LDS per workgroup — how a workgroup's waves spread over the SIMDs. */
int rs_diag_wave_slots(int grid, int block, int lds_bytes, uint32_t* out, rs_stream_t stream);
/* rs_diag_mfma_chain: every wave issues n v_mfma_f32_16x16x4_f32 as `chains`
 * (1, 2, 4) independent accumulation chains; cyc[3 wave + {0, 1, 2}] = its
 * start / end s_memtime and its HW_ID (SIMD in bits 5:4), so the host can time
 * each SIMD's window from its first wave's start to its last wave's end. */
int rs_diag_mfma_chain(int grid, int block, int n, int chains, unsigned long long* cyc, float* sink,
                       rs_stream_t stream);
/* rs_diag_icache: 2048 FMAs per wave as a loop (unroll 0) or straight-line
 * code (unroll 1), run twice in one launch; cyc[2 wave + pass] = cycles.     */
int rs_diag_icache(int grid, int block, int unroll, unsigned long long* cyc, float* sink, rs_stream_t stream);

/* --------------------------------------------------------- embedding (a3)
 * Replaces EmbedLayer.call (layer/core.py:273-280) + the dense/sparse concat of
 * DeepFM.call / DCN.call (model/deepFM.py:24-26, model/dcn.py:25-27):
 *   out[b, 0:nd]               = dense[b, 0:nd]
 *   out[b, nd + c*k + j]       = table[field_offsets[c] + id(b,c), j]
 * One contiguous table holds every field's Keras `Embedding` matrix stacked
 * (field c occupies rows [field_offsets[c], field_offsets[c]+field_vocab[c])).
 * nd may be 0 (dense may then be NULL): the result is EmbedLayer's [B, F*k].
 * field_offsets / field_vocab are device int64[F].                          */
int rs_embed_gather(const void* ids, int id_kind, int64_t id_stride,
                    const float* dense, int64_t dense_stride, int nd,
                    const float* table, const int64_t* field_offsets,
                    const int64_t* field_vocab, int n_fields, int k,
                    float* out, int64_t out_stride, int64_t batch,
                    int* err_flag, rs_stream_t stream);

/* ---------------------------------------------------- FM second order (a5)
 * FMLayer.call (layer/interaction.py:106-114) on x = [dense | emb] with
 * d = nd + F*k, weights w0:(1,), w1:(d,1), v:(d,kfm):
 *   y[b] = x@w1 + w0 + 0.5*sum_f((x@v)_f^2 - (x^2 @ v^2)_f)
 * The kernels consume a packed weight image built once per weight set by
 * rs_fm_prepare (MFMA operand order + per-row squared norms of v); query its
 * size in floats with rs_fm_prepared_size.                                   */
int64_t rs_fm_prepared_size(int nd, int n_fields, int k, int kfm);
int rs_fm_prepare(const float* w1, const float* v, int nd, int n_fields, int k,
                  int kfm, float* prepared, rs_stream_t stream);
/* The kernarg-metadata kernels (below) have instantiations specialised for
 * one shape, with the packed image's geometry as compile-time constants.
 * Host-only query of what their launchers decide for a shape: 1 = it is the
 * specialised shape and the compile-time geometry equals the packed image's
 * (the specialised kernels run), 0 = another shape, -1 = the shape, but the
 * geometry differs (both: the generic kernels, run-time geometry).           */
int rs_embed_fm_ct_geom(int nd, int n_fields, int k, int kfm);

/* Fused EmbedLayer + concat + FMLayer (the headline kernel; DeepFM semantics,
 * model/deepFM.py:24-28).  logit[b] = FMLayer(x)[b]; if x_out != NULL the
 * concatenated x[B,d] (row stride d) is also written for the DNN tower.      */
int rs_embed_fm_fwd(const void* ids, int id_kind, int64_t id_stride,
                    const float* dense, int64_t dense_stride, int nd,
                    const float* table, const int64_t* field_offsets,
                    const int64_t* field_vocab, int n_fields, int k,
                    const float* prepared, const float* w0, int kfm,
                    float* logit, float* x_out, int64_t batch, int* err_flag,
                    rs_stream_t stream);
/* The same with the field metadata also given on the HOST (read at call
 * time, copied into the launch: graph capture keeps the values of the
 * capturing call).  For n_fields <= 32 and batch <= 8192 the kernel then
 * reads (offset, vocab) through scalar kernel-argument loads and each wave
 * loads its own fields' ids — no workgroup id tile, no barrier; otherwise
 * (or with a kernel option other than 0 set) it is rs_embed_fm_fwd.  The
 * host arrays must equal the device ones.                                    */
int rs_embed_fm_fwd_hm(const void* ids, int id_kind, int64_t id_stride,
                       const float* dense, int64_t dense_stride, int nd,
                       const float* table, const int64_t* field_offsets,
                       const int64_t* field_vocab,
                       const int64_t* field_offsets_host,
                       const int64_t* field_vocab_host, int n_fields, int k,
                       const float* prepared, const float* w0, int kfm,
                       float* logit, float* x_out, int64_t batch, int* err_flag,
                       rs_stream_t stream);

/* FMLayer on an arbitrary dense x[B,n] (layer/interaction.py:106-114), e.g.
 * the FM model's one-hot input (model/fm.py:19-23).  `prepared` comes from
 * rs_fm_prepare(w1, v, n, 0, 0, kfm, ...).                                   */
int rs_fm_fwd(const float* x, int64_t x_stride, int n, const float* prepared,
              const float* w0, int kfm, float* logit, int64_t batch,
              rs_stream_t stream);

/* FM model on the compact form of its one-hot input (model/fm.py:19-23 with
 * utils/dataset.py:47-48): x = [dense(nd) | onehot], where the one-hot block
 * has exactly one 1 per field at column nd + field_offsets[c] + id(b,c).
 * Gathers rows of v and w1 instead of multiplying by zeros.                  */
int rs_fm_onehot_fwd(const void* ids, int id_kind, int64_t id_stride,
                     const float* dense, int64_t dense_stride, int nd,
                     const int64_t* field_offsets, const int64_t* field_vocab,
                     int n_fields, const float* w1, const float* w0,
                     const float* v, int kfm, float* logit, int64_t batch,
                     int* err_flag, rs_stream_t stream);

/* ------------------------------------------------------ DCN CrossNet (a9)
 * CrossLayer.call (layer/interaction.py:75-83):
 *   x_{l+1} = x0 * (x_l^T w_l) + b_l + x_l,  l = 0..L-1,  out = x_L
 * w, b: [L, d] (Keras shapes (d,1) each, stacked).  The L contractions
 * x0^T w_l run on fp32 MFMA; `prepared` (rs_cross_prepared_size floats) holds
 * the packed weights and the sample-independent bias terms.  rs_cross_fwd:
 * L <= 32, d <= 2304, and d <= 2295 with more than 16 layers (the 16-sample
 * tile and the waves' partial products share 160 KB of LDS).                 */
int64_t rs_cross_prepared_size(int d, int n_layers);
int rs_cross_prepare(const float* w, const float* b, int d, int n_layers,
                     float* prepared, rs_stream_t stream);
int rs_cross_fwd(const float* x0, int64_t x_stride, int d, int n_layers,
                 const float* prepared, float* out, int64_t out_stride,
                 int64_t batch, rs_stream_t stream);

/* Fused DCN input + CrossNet: x0 = [dense | EmbedLayer(ids)] (model/dcn.py:
 * 24-27, layer/core.py:273-280) is assembled in LDS — never written to HBM —
 * and out = CrossLayer(x0) (layer/interaction.py:75-83).  Gather arguments as
 * rs_embed_gather; prepared from rs_cross_prepare(d = nd + F*k).  k % 4 == 0,
 * 1..128 fields, d <= 1600.  Out-of-range ids set *err_flag, rows read 0.    */
int rs_embed_cross_fwd(const void* ids, int id_kind, int64_t id_stride,
                       const float* dense, int64_t dense_stride, int nd,
                       const float* table, const int64_t* field_offsets,
                       const int64_t* field_vocab, int n_fields, int k,
                       int n_layers, const float* prepared, float* out,
                       int64_t out_stride, int64_t batch, int* err_flag,
                       rs_stream_t stream);
/* The same with the fields' (offset, vocab) also on the host: at k = 16 and
 * <= 32 fields they travel as kernel arguments and the rows come in through
 * the headline kernel's front end (per-wave field ids, no id tile; DESIGN.md
 * 4.2); otherwise identical to rs_embed_cross_fwd.  Bit-identical outputs. */
int rs_embed_cross_fwd_hm(const void* ids, int id_kind, int64_t id_stride,
                          const float* dense, int64_t dense_stride, int nd,
                          const float* table, const int64_t* field_offsets,
                          const int64_t* field_vocab,
                          const int64_t* field_offsets_host,
                          const int64_t* field_vocab_host, int n_fields, int k,
                          int n_layers, const float* prepared, float* out,
                          int64_t out_stride, int64_t batch, int* err_flag,
                          rs_stream_t stream);

/* Fused DCN forward (model/dcn.py:24-34) in one launch: x0 in LDS, CrossNet
 * folded into its contraction, the DNN tower on the same tile, head
 * sigmoid(Dense1([x_L | dnn])).  cross_prepared: rs_cross_prepare over
 * n_cross + 1 columns — w_0..w_{L-1} then the output Dense's cross half
 * w_o[:d] (bias row 0) — so the cross branch's logit is alpha_L (x0.w_o) +
 * beta_L.w_o without forming x_L.  mlp_prepared: rs_mlp_prepare of the DNN
 * hidden layers plus ONE folded last layer (W_last w_o[d:], b_last w_o[d:] +
 * b_o), dims[n_layers] == 1, no input permutation.  rs_dcn_fused_ok: shape
 * supported (k % 4 == 0, 1..128 fields, n_cross <= 31).                    */
int rs_dcn_fused_ok(int nd, int n_fields, int k, int n_cross, int n_layers,
                    const int* dims);
int rs_dcn_fwd(const void* ids, int id_kind, int64_t id_stride,
               const float* dense, int64_t dense_stride, int nd,
               const float* table, const int64_t* field_offsets,
               const int64_t* field_vocab, int n_fields, int k, int n_cross,
               const float* cross_prepared, int n_layers, const int* dims,
               const int* acts, const float* mlp_prepared, float* out,
               int64_t batch, int* err_flag, rs_stream_t stream);
/* rs_dcn_fwd with host field metadata (kernel-argument front end, as
 * rs_embed_cross_fwd_hm).  Bit-identical outputs. */
int rs_dcn_fwd_hm(const void* ids, int id_kind, int64_t id_stride,
                  const float* dense, int64_t dense_stride, int nd,
                  const float* table, const int64_t* field_offsets,
                  const int64_t* field_vocab, const int64_t* field_offsets_host,
                  const int64_t* field_vocab_host, int n_fields, int k,
                  int n_cross, const float* cross_prepared, int n_layers,
                  const int* dims, const int* acts, const float* mlp_prepared,
                  float* out, int64_t batch, int* err_flag, rs_stream_t stream);

/* ----------------------------------------------- PNN inner product (a11)
 * InnerProductLayer.call (layer/interaction.py:170-183) on e[B,F,k]:
 *   out[b,p] = <e[b,i_p,:], e[b,j_p,:]>, pairs (i<j) in row-major order.
 * out row stride is out_stride (>= F(F-1)/2).  k <= 64.  n_fields <= 513
 * (with rs_embed_inner_fwd and rs_embed_inner_fwd_hm): outside the MFMA path
 * (k in {4,8,16,32,64}, 2..128 fields, 2..64 from ids) one thread of 256 owns
 * the Gram rows g and F-2-g, g < F/2, so F/2 <= 256; a sample's F*k floats
 * must also fit in 150 KB of LDS.  A larger shape returns RS_ERR_ARG and
 * launches nothing.                                                         */
int rs_inner_product_fwd(const float* emb, int n_fields, int k, float* out,
                         int64_t out_stride, int64_t batch, rs_stream_t stream);

/* Fused gather + flatten + inner product: writes the PNN DNN input
 * out[b] = [flat_emb (F*k) | inner (F(F-1)/2)] (model/pnn.py:34-41).       */
int rs_embed_inner_fwd(const void* ids, int id_kind, int64_t id_stride,
                       const float* table, const int64_t* field_offsets,
                       const int64_t* field_vocab, int n_fields, int k,
                       float* out, int64_t out_stride, int64_t batch,
                       int* err_flag, rs_stream_t stream);
/* rs_embed_inner_fwd with host field metadata (kernel-argument front end at
 * k = 16, <= 32 fields).  Bit-identical outputs. */
int rs_embed_inner_fwd_hm(const void* ids, int id_kind, int64_t id_stride,
                          const float* table, const int64_t* field_offsets,
                          const int64_t* field_vocab,
                          const int64_t* field_offsets_host,
                          const int64_t* field_vocab_host, int n_fields, int k,
                          float* out, int64_t out_stride, int64_t batch,
                          int* err_flag, rs_stream_t stream);

/* OuterProductLayer (layer/interaction.py:186-215): out[b,p] =
 * sum_{a,j} e[b,row_p,j] W[a,p,j] e[b,col_p,a] with W the Keras weight
 * [k, P, k], pairs in the reference's row-major i<j order.  rs_outer_prepare
 * packs W into per-lane MFMA fragments (rs_outer_prepared_size floats; k in
 * {4,8,16,32,64}, 2..128 fields).  rs_outer_product_fwd: emb [B,F,k] -> out
 * [B,P].  rs_embed_product_fwd: PNN's DNN input (model/pnn.py:32-48) from ids
 * in one launch — out[b] = [flat_emb (F*k) | inner (P, if inner) | outer (P,
 * if outer_prepared)]; mode 'inner' / 'outer' / 'both'.                      */
int64_t rs_outer_prepared_size(int n_fields, int k);
int rs_outer_prepare(const float* W, int n_fields, int k, float* prepared,
                     rs_stream_t stream);
int rs_outer_product_fwd(const float* emb, int n_fields, int k,
                         const float* outer_prepared, float* out,
                         int64_t out_stride, int64_t batch, rs_stream_t stream);
int rs_embed_product_fwd(const void* ids, int id_kind, int64_t id_stride,
                         const float* table, const int64_t* field_offsets,
                         const int64_t* field_vocab, int n_fields, int k,
                         int inner, const float* outer_prepared, float* out,
                         int64_t out_stride, int64_t batch, int* err_flag,
                         rs_stream_t stream);
/* rs_embed_product_fwd with host field metadata (as rs_embed_inner_fwd_hm). */
int rs_embed_product_fwd_hm(const void* ids, int id_kind, int64_t id_stride,
                            const float* table, const int64_t* field_offsets,
                            const int64_t* field_vocab,
                            const int64_t* field_offsets_host,
                            const int64_t* field_vocab_host, int n_fields, int k,
                            int inner, const float* outer_prepared, float* out,
                            int64_t out_stride, int64_t batch, int* err_flag,
                            rs_stream_t stream);
/* The same row from a GIVEN emb [B,F,k] in one launch: out[b] = [flat (F*k) |
 * inner (P, if inner) | outer (P, if outer_prepared)] — PNN's DNN input when
 * the product layers run on z = concat([embed, fgcnn_out]) (model/pnn.py:
 * 33-48).  From given embeddings (this entry, rs_inner_product_fwd,
 * rs_outer_prepare*, rs_outer_product_fwd) the MFMA path takes 2..128 fields;
 * from ids (rs_embed_*) 2..64.  As many samples per workgroup as fit in 96
 * KB of LDS (per sample F*k + 4 + pairs floats; the largest shape, 128
 * fields, k 64, inner and outer, is 97,808 bytes: one sample).  A tile past
 * that budget would return RS_ERR_ARG and launch nothing.                  */
int rs_product_fwd(const float* emb, int n_fields, int k, int inner,
                   const float* outer_prepared, float* out, int64_t out_stride,
                   int64_t batch, rs_stream_t stream);

/* ---------------------------------------------- FGCNN conv stack (a12)
 * FGCNNLayer.call (layer/interaction.py:245-258) on e [B, F, k], x = e[...,
 * None]; layer i = 0..n_layers-1 on its input map [H, k, Cin] (H_0 = F,
 * Cin_0 = 1):
 *   Conv2D(filters[i], (kernel_width[i], 1), 'same', tanh): along the field
 *     axis only, kernel conv_w[i] [kw, 1, Cin, Cout] (Keras shape), bias
 *     conv_b[i] [Cout]; TF 'same' pads (kw-1)/2 rows before, the rest after;
 *   MaxPool2D((pooling_width[i], 1)): H' = H / pw, trailing rows dropped.
 * The pooled map [H', k, Cout] is the next layer's input and is written, in
 * Keras Flatten order, to workspace[b, off_i : off_i + H'*k*Cout] (off_i = the
 * sum of the earlier layers' sizes; rows ws_stride floats apart) — the x of
 * the layer's recombination Dense (rs_dense_fwd with y inside z at the
 * layer's column offset).  All layers run in ONE launch; the maps stay in LDS.
 * rs_fgcnn_workspace_size: floats per sample (the sum over layers), or -1 for
 * a configuration outside 1..4 layers, 1..32 filters, kernel_width >= 1,
 * pooling_width >= 1, k in {4,8,16,32,64}, every H' >= 1 and the per-sample
 * LDS tile (padded maps + the staged weights <= 128 KB).
 * filters / kernel_width / pooling_width: host int[n_layers]; conv_w / conv_b:
 * host arrays of device pointers.
 * rs_embed_fgcnn_conv_fwd: the same from ids (gather arguments as
 * rs_embed_inner_fwd: an out-of-range id reads a zero row and sets
 * *err_flag); the gathered rows also go to z[b, 0:F*k] (rows z_stride floats
 * apart; z may be NULL), so PNN needs no separate gather.  Bit-identical to
 * rs_fgcnn_conv_fwd on the gathered rows.                                   */
int64_t rs_fgcnn_workspace_size(int n_fields, int k, int n_layers,
                                const int* filters, const int* kernel_width,
                                const int* pooling_width);
int rs_fgcnn_conv_fwd(const float* emb, int n_fields, int k, int n_layers,
                      const int* filters, const int* kernel_width,
                      const int* pooling_width, const float* const* conv_w,
                      const float* const* conv_b, float* workspace,
                      int64_t ws_stride, int64_t batch, rs_stream_t stream);
int rs_embed_fgcnn_conv_fwd(const void* ids, int id_kind, int64_t id_stride,
                            const float* table, const int64_t* field_offsets,
                            const int64_t* field_vocab, int n_fields, int k,
                            int n_layers, const int* filters,
                            const int* kernel_width, const int* pooling_width,
                            const float* const* conv_w,
                            const float* const* conv_b, float* workspace,
                            int64_t ws_stride, float* z, int64_t z_stride,
                            int64_t batch, int* err_flag, rs_stream_t stream);

/* ---------------------------------------------- DIN attention unit (a13)
 * Attention.call (layer/interaction.py:369-406), 'prelu' mode:
 *   e_t   = [q, key_t, q-key_t, q*key_t]                         (4k)
 *   h1_t  = PReLU_{alpha1[t]}(e_t @ W1 + b1)                     (H1)
 *   h2_t  = PReLU_{alpha2[t]}(h1_t @ W2 + b2)                    (H2)
 *   s_t   = h2_t @ w3 + b3;  s_t = -4294967296 where mask[b,t]==0
 *   out   = softmax_t(s) @ value                                 (k)
 * W1 [4k,H1], W2 [H1,H2], w3 [H2], alpha1 [T,H1], alpha2 [T,H2] (Keras
 * PReLU inside Dense on a 3-D input: alpha shape input_shape[1:]).
 * `mask` is float [B,T] (0 = padded).  Supported: k in {4,8,16,32},
 * H1,H2 <= 128.                                                              */
int rs_din_attention_fwd(const float* query, const float* keys,
                         const float* values, const float* mask, int T, int k,
                         const float* W1, const float* b1, const float* alpha1,
                         int H1, const float* W2, const float* b2,
                         const float* alpha2, int H2, const float* w3,
                         const float* b3, float* out, int64_t batch,
                         rs_stream_t stream);

/* Attention.call 'dice' mode (layer/interaction.py:363-364, 410-425): the
 * activation stack is n_dice Dice layers applied to e_t (no Dense), then
 * Dense(1).  Dice at inference: xhat=(x-mean)/sqrt(var+eps), p=sigmoid(xhat),
 * y = alpha*(1-p)*x + p*x; per-layer mean/var/alpha are [n_dice, 4k].        */
int rs_din_attention_dice_fwd(const float* query, const float* keys,
                              const float* values, const float* mask, int T,
                              int k, int n_dice, const float* dice_alpha,
                              const float* dice_mean, const float* dice_var,
                              float dice_eps, const float* w_out,
                              const float* b_out, float* out, int64_t batch,
                              rs_stream_t stream);

/* Attention.call 'prelu' at any depth (layer/interaction.py:355-406 with
 * len(hidden_units) = n_layers, any H, k <= 64 or larger): e = [q, key_t,
 * q-key_t, q*key_t] per (b, t) row, Dense(hidden[l], PReLU()) with alpha
 * [T, hidden[l]] as fp32 MFMA GEMMs over the B*T rows, Dense(1), masked
 * softmax, weighted sum of the values.  W[l] (in, out) Keras orientation,
 * b[l] [hidden[l]], alpha[l] [T, hidden[l]] (device pointers in host
 * arrays).  workspace: rs_din_attention_gen_workspace_size bytes (device).   */
int64_t rs_din_attention_gen_workspace_size(int64_t batch, int T, int k,
                                            int n_layers, const int* hidden);
int rs_din_attention_gen_fwd(const float* query, const float* keys,
                             const float* values, const float* mask, int T,
                             int k, int n_layers, const int* hidden,
                             const float* const* W, const float* const* b,
                             const float* const* alpha, const float* w_out,
                             const float* b_out, float* out, int64_t batch,
                             void* workspace, int64_t workspace_bytes,
                             rs_stream_t stream);

/* DIN attention straight from behaviour ids (model/din.py:56-80 + Attention
 * 'prelu', layer/interaction.py:355-406): key = value = table[hist[b,t]],
 * query = table[cand[b]], mask = hist != 0.  At the reference's (80, 40)
 * widths ONE launch (din_fused: every position's PReLU alphas and W2 staged
 * once per workgroup of 8 samples, layer 1 regrouped per sample as
 * q(Wq+Wd) + key(Wk-Wd+diag(q)Wp), per-tile online-softmax partials merged
 * per sample — the scores never reach HBM); other widths, or
 * RS_OPT_DIN_KERNEL 1, two launches (scores, then the masked softmax pool).
 * prepared: rs_din_prepare (k in {4,8,16}, H1 <= 128, H2 <= 64); scores: a
 * caller-owned [B, T] fp32 workspace (untouched by the one-launch form);
 * out [B, k] with rows out_stride
 * floats apart (>= k: DIN.call writes straight into its concat).  T <= 1024.
 * OOR ids set *err_flag.                                                   */
int64_t rs_din_prepared_size(int T, int k, int H1, int H2);
int rs_din_prepare(const float* W1, const float* b1, const float* alpha1,
                   int H1, const float* W2, const float* b2,
                   const float* alpha2, int H2, const float* w3,
                   const float* b3, int T, int k, float* prepared,
                   rs_stream_t stream);
int rs_din_attention_ids_fwd(const void* hist, int id_kind, int64_t hist_stride,
                             const void* cand, int64_t cand_stride, int T,
                             int k, const float* table, int64_t vocab, int H1,
                             int H2, const float* prepared, float* scores,
                             float* out, int64_t out_stride, int64_t batch,
                             int* err_flag, rs_stream_t stream);
/* ... and the candidate rows table[cand] into cand_out [B, k] (rows
 * cand_out_stride floats apart; an out-of-range id writes a zero row and sets
 * *err_flag), the copy DIN.call concatenates beside the pooled rows
 * (model/din.py:78-79,84-85): the same launch, no separate candidate gather.   */
int rs_din_attention_ids_cand_fwd(const void* hist, int id_kind,
                                  int64_t hist_stride, const void* cand,
                                  int64_t cand_stride, int T, int k,
                                  const float* table, int64_t vocab, int H1,
                                  int H2, const float* prepared, float* scores,
                                  float* out, int64_t out_stride,
                                  float* cand_out, int64_t cand_out_stride,
                                  int64_t batch, int* err_flag,
                                  rs_stream_t stream);

/* DIN.call (model/din.py:56-95) in ONE launch: the attention unit of
 * rs_din_attention_ids_cand_fwd, then BatchNormalization (in_scale / in_shift,
 * as rs_mlp_affine_fwd) + the PReLU tower + Dense(1, sigmoid) of
 * rs_mlp_affine_pieces_fwd over the input [pooled (k) | cand rows (k) |
 * pieces] — the pieces must cover columns 2k .. dims[0]-1 (in_cols >= 2k;
 * n_pieces = 0 when dims[0] == 2k) —
 * writing y [B] (rows y_stride apart).  Bit-identical to those two launches.
 * pooled (optional, rows pooled_stride apart) also receives the attention
 * output.  rs_din_forward_ids_supported: 1 when the shape takes the fused
 * launch (the reference's (80, 40) attention, a 256-unit first layer and the
 * 128 -> 64 -> 1 tail, dims[0] <= 64), else 0 (the caller keeps two launches).
 * Replaces DIN.call's attention + concat + bn + dense_layer + out_layer. */
int rs_din_forward_ids_supported(int T, int k, int H1, int H2, int n_layers,
                                 const int* dims);
int rs_din_forward_ids(const void* hist, int id_kind, int64_t hist_stride,
                       const void* cand, int64_t cand_stride, int T, int k,
                       const float* table, int64_t vocab, int H1, int H2,
                       const float* att_prepared, float* pooled,
                       int64_t pooled_stride, const float* in_scale,
                       const float* in_shift, int n_layers, const int* dims,
                       const int* acts, const float* tower_prepared, float* y,
                       int64_t y_stride, int n_pieces, const int* widths,
                       const int* in_cols, const int* kinds,
                       const void* const* srcs, const int64_t* src_strides,
                       const float* const* tables, const int64_t* vocabs,
                       int64_t batch, int* err_flag, rs_stream_t stream);

/* ------------------------------------------------ concat pieces (a15, a3)
 * One launch for the concat pieces that live in different tables: piece p
 * writes widths[p] columns of out [B, *] (rows out_stride floats apart)
 * starting at out_cols[p].  kinds[p] = RS_ID_* : a sparse feature, one id
 * per sample (srcs[p], src_strides[p] elements apart) looked up in
 * tables[p] [vocabs[p], widths[p]] (Keras Embedding; an out-of-range id
 * writes a zero row and sets *err_flag); kinds[p] = -1: dense fp32 values
 * [B, widths[p]] copied as they are.  DIN.call's other sparse embeddings and
 * dense features (model/din.py:64-69,84-85).  1..16 pieces.                      */
int rs_concat_pieces(int n_pieces, const int* widths, const int* out_cols,
                     const int* kinds, const void* const* srcs,
                     const int64_t* src_strides, const float* const* tables,
                     const int64_t* vocabs, float* out, int64_t out_stride,
                     int64_t batch, int* err_flag, rs_stream_t stream);

/* --------------------------------------------------- dense tower (a7, a15)
 * Keras Dense: y = act(x @ W + bias), W:[K,N] (Keras (in,out) orientation),
 * fp32 MFMA.  alpha: per-column PReLU slope (RS_ACT_PRELU only).            */
int rs_dense_fwd(const float* x, int64_t x_stride, const float* W,
                 const float* bias, const float* alpha, int act, float* y,
                 int64_t y_stride, int64_t M, int K, int N, rs_stream_t stream);

/* ------------------------------------------------ fused MLP tower (a7, §8f)
 * The whole DNNLayer (layer/interaction.py:30-46: hidden Dense(h_i, act) then
 * Dense(output_dim)) in one launch; activations stay in LDS.
 * dims[0..n_layers]: input width then each layer's units (each <= 1024);
 * W[l]: Keras kernel [dims[l], dims[l+1]]; bias[l], alpha[l] (PReLU) may be
 * NULL.  in_rows (device int32 [roundup(dims[0],16)], may be NULL): LDS
 * input column p reads Keras kernel row in_rows[p] (-1 = none), so a fused
 * producer can keep its own column order.  rs_mlp_prepared_size returns
 * floats (-1 on bad dims).                                                   */
int64_t rs_mlp_prepared_size(int n_layers, const int* dims);
int rs_mlp_prepare(int n_layers, const int* dims, const float* const* W,
                   const float* const* bias, const float* const* alpha,
                   const int32_t* in_rows, float* prepared, rs_stream_t stream);
/* head 0: y[M, dims[n_layers]] = tower(x).  head 1 (dims[n_layers] == 1):
 * y[m] = sigmoid(c0 * tower(x)[m] + c1 * extra[m]) — the DeepFM head
 * model/deepFM.py:30 (extra = FM logit, c0 = c1 = 0.5); extra may be NULL.
 * acts[l]: rs_act per layer (hidden: the DNNLayer activation; last: NONE).  */
int rs_mlp_fwd(const float* x, int64_t x_stride, int n_layers, const int* dims,
               const int* acts, const float* prepared, float* y,
               int64_t y_stride, int head, const float* extra, float c0,
               float c1, int64_t batch, rs_stream_t stream);
/* ... with an inference BatchNormalization on the input folded into the
 * tile staging: column c enters the tower as x[m, c] * in_scale[c] +
 * in_shift[c] (rs_affine_act's arithmetic; DIN.call's bn_layer before the
 * DNN, model/din.py:89), so the normalised concat never reaches HBM.        */
int rs_mlp_affine_fwd(const float* x, int64_t x_stride, const float* in_scale,
                      const float* in_shift, int n_layers, const int* dims,
                      const int* acts, const float* prepared, float* y,
                      int64_t y_stride, int head, const float* extra, float c0,
                      float c1, int64_t batch, rs_stream_t stream);
/* ... and some input columns read straight from their sources instead of x:
 * the concat pieces of rs_concat_pieces (widths / kinds / srcs / strides /
 * tables / vocabs as there; in_cols = the input column of each piece's first
 * column), e.g. DIN.call's other sparse embeddings and dense features
 * (model/din.py:64-69,84-85) beside the pooled attention — the concat is
 * never written and needs no launch of its own.  x (rows x_stride apart)
 * provides every other column (NULL if the pieces cover them all).  At most
 * 64 input columns; an out-of-range id reads a zero row and sets err_flag. */
int rs_mlp_affine_pieces_fwd(const float* x, int64_t x_stride,
                             const float* in_scale, const float* in_shift,
                             int n_layers, const int* dims, const int* acts,
                             const float* prepared, float* y, int64_t y_stride,
                             int head, const float* extra, float c0, float c1,
                             int64_t batch, int n_pieces, const int* widths,
                             const int* in_cols, const int* kinds,
                             const void* const* srcs,
                             const int64_t* src_strides,
                             const float* const* tables, const int64_t* vocabs,
                             int* err_flag, rs_stream_t stream);

/* ------------------------------------- residual tower (DeepCrossing, a16)
 * ResLayer.call (layer/interaction.py:261-278) on x [B, d]:
 *   h = x;  h = relu(h @ W_i + b_i) for each hidden width;  h = h @ W_out + b_out
 *   (W_out [last, d], no activation);  result = relu(x + h)
 * stacked n_units times, each unit with its own weights but the same widths
 * (model/deepCrossing.py:15-32), in ONE launch; a 16-sample tile stays in LDS
 * from the input to the result and the skip operand stays in registers.
 * hidden: host int[n_hidden], n_hidden 1..4; n_units 1..16; d and every
 * width 1..1024.  rs_res_tower_ok: 1 when the shape is supported (the real
 * LDS geometry), else 0.
 * prepared (rs_res_tower_prepared_size floats, -1 on a bad shape) =
 *   n_units * sum_l (Kp_l * Np_l + Np_l) + head * (roundup(d, 16) + 16)
 * over the n_hidden + 1 layers of a unit, Kp / Np = a layer's input / output
 * width rounded up to 16.  rs_res_tower_prepare packs it: W / bias are host
 * arrays of n_units * (n_hidden + 1) device pointers, unit-major (Keras
 * kernels [in, out]; bias, or any bias[i], may be NULL = zeros); head_w [d],
 * head_b [1] (NULL = 0) are the model's Dense(1) — head_w NULL packs no head.
 * rs_res_tower_fwd: head 0: y [B, d] (rows y_stride apart) = the last unit's
 * output; head 1: y[b * y_stride] = sigmoid(x_L[b] . head_w + head_b)
 * (prepared must hold the head; an image packed with the head serves head 0
 * too).
 * rs_deepcrossing_fwd: DeepCrossing.call from the ids — x = [dense (nd) |
 * EmbedLayer rows (n_fields * k)] is staged straight into the input tile (the
 * concat is never written; gather arguments as rs_embed_gather, an
 * out-of-range id reads a zero row and sets *err_flag), then the units and
 * the head: out [B]; x_last (optional, [B, d], rows x_last_stride apart)
 * receives the last unit's output.  prepared must hold the head.
 * Bit-identical to rs_res_tower_fwd on the same x.                          */
int rs_res_tower_ok(int d, int n_hidden, const int* hidden, int n_units);
int64_t rs_res_tower_prepared_size(int d, int n_hidden, const int* hidden,
                                   int n_units, int head);
int rs_res_tower_prepare(int d, int n_hidden, const int* hidden, int n_units,
                         const float* const* W, const float* const* bias,
                         const float* head_w, const float* head_b,
                         float* prepared, rs_stream_t stream);
int rs_res_tower_fwd(const float* x, int64_t x_stride, int d, int n_hidden,
                     const int* hidden, int n_units, const float* prepared,
                     int head, float* y, int64_t y_stride, int64_t batch,
                     rs_stream_t stream);
int rs_deepcrossing_fwd(const void* ids, int id_kind, int64_t id_stride,
                        const float* dense, int64_t dense_stride, int nd,
                        const float* table, const int64_t* field_offsets,
                        const int64_t* field_vocab, int n_fields, int k,
                        int n_hidden, const int* hidden, int n_units,
                        const float* prepared, float* out, float* x_last,
                        int64_t x_last_stride, int64_t batch, int* err_flag,
                        rs_stream_t stream);

/* Training the residual stack (DeepCrossing.train_step).  Every entry takes
 * exactly the shapes rs_res_tower_ok accepts, launches nothing for batch 0,
 * is stream-ordered and graph-capturable.
 * saved (rs_res_tower_saved_size floats, -1 on a bad shape or batch < 0) =
 *   x_0 [B, d], then unit-major, layer-major, dense row-major a_{u,l}
 *   [B, N_l]: a_{u,l} = the relu output of hidden layer l (N_l = hidden[l]),
 *   a_{u,n_hidden} = x_{u+1}, the unit's result (N = d);
 *   B * (d + n_units * (sum(hidden) + d)) floats.
 * rs_res_tower_train_fwd / rs_deepcrossing_train_fwd: rs_res_tower_fwd(head
 * 1) / rs_deepcrossing_fwd, bit-identical, that also store `saved` (x_0 from
 * the staged tile: in the ids form the only place [dense | rows] is written)
 * and the head's logit [B]; out [B] = sigmoid(logit).  prepared must hold the
 * head.
 * The backward image (rs_res_tower_bwd_prepared_size floats: the forward's
 * formula for `hidden` reversed, with the head slot) holds, for the units in
 * the order the backward visits them (last first), chain layer l = W_{n_hidden
 * - l}^T in the forward's B-fragment layout, no biases, and head_w (NULL =
 * zeros: an image for the dy form only).  W: n_units * (n_hidden + 1) device
 * pointers in the forward's order (rs_res_tower_prepare).
 * rs_res_tower_bwd: one launch over 16-sample tiles.  Exactly one of dy
 * [B, d] (rows dy_stride apart: dL/dx_U) and g [B] (dL/dx_U = g[b] * head_w)
 * is given.  deltas = the layout of saved without x_0: delta_{u,l} = dL/d(pre-
 * activation of layer l of unit u); delta_{u,n_hidden} = dL/dx_{u+1} [x_{u+1}
 * > 0].  dx0 [B, d] (rows dx0_stride apart) = dL/dx_0.  Masks are
 * post-activation > 0 (rs_gemm's mask epilogue).  Deterministic; a row's
 * result does not depend on the batch.                                       */
int64_t rs_res_tower_saved_size(int d, int n_hidden, const int* hidden,
                                int n_units, int64_t batch);
int rs_res_tower_train_fwd(const float* x, int64_t x_stride, int d,
                           int n_hidden, const int* hidden, int n_units,
                           const float* prepared, float* saved, float* out,
                           float* logit, int64_t batch, rs_stream_t stream);
int rs_deepcrossing_train_fwd(const void* ids, int id_kind, int64_t id_stride,
                              const float* dense, int64_t dense_stride, int nd,
                              const float* table, const int64_t* field_offsets,
                              const int64_t* field_vocab, int n_fields, int k,
                              int n_hidden, const int* hidden, int n_units,
                              const float* prepared, float* saved, float* out,
                              float* logit, int64_t batch, int* err_flag,
                              rs_stream_t stream);
int64_t rs_res_tower_bwd_prepared_size(int d, int n_hidden, const int* hidden,
                                       int n_units);
int rs_res_tower_prepare_bwd(int d, int n_hidden, const int* hidden,
                             int n_units, const float* const* W,
                             const float* head_w, float* prepared,
                             rs_stream_t stream);
int rs_res_tower_bwd(const float* saved, int d, int n_hidden,
                     const int* hidden, int n_units, const float* prepared_bwd,
                     const float* dy, int64_t dy_stride, const float* g,
                     float* deltas, float* dx0, int64_t dx0_stride,
                     int64_t batch, rs_stream_t stream);

/* ----------------------- multi-gate mixture of experts (MMOE, a18), forward
 * mmoe_layer.call (layer/interaction.py:479-509) on x [B, d], rows x_stride
 * apart, with H = hidden, E = n_experts, T = n_tasks:
 *   expert[b, h, e] = relu(x[b] . expert_matrix[:, h, e] + expert_bias[h, e])
 *   g_t[b, :]       = softmax(x[b] @ gate_matrix_t + gate_bias_t)   (over E)
 *   mix_t[b, h]     = sum_e g_t[b, e] * expert[b, h, e]
 * and, with n_tower_layers >= 1, MMOE.call (model/mmoe.py:24-32): task t's
 * tower_layer (layer/interaction.py:512-523: Dense(tower_dims[i + 1],
 * tower_acts[i]) per layer, the last one the linear Dense(output_dim)) on
 * mix_t — ONE launch over 16-sample tiles; expert outputs, gates, mixes and
 * tower activations stay in LDS.  The softmax subtracts the row maximum; every
 * sum has one fixed order (e ascending), a row's result does not depend on the
 * batch.
 * tower_dims: host int[n_tower_layers + 1], tower_dims[0] == hidden, the last
 * = output_dim (may be NULL when n_tower_layers == 0); all towers share the
 * widths and tower_acts (host int[n_tower_layers]: RS_ACT_NONE, RS_ACT_RELU
 * or RS_ACT_SIGMOID) but have their own weights.
 * Caps: d, hidden and every tower width 1..1024; 1 <= E <= 16; 1 <= T <= 8;
 * roundup((H + T) * E, 16) <= 1024; 0..4 tower layers; and the tile must fit
 * the LDS: with maxw = max(roundup(d, 16), E * (H | 1) + T * E,
 * T * roundup(w, 16) over w in {H, tower widths}), 4 * (32 * (roundup(maxw,
 * 64) + 8) + 4096) <= 160 KiB.  rs_mmoe_ok: 1 when the shape is supported
 * (that geometry), else 0 — the reference's constructors
 * (layer/interaction.py:430-436, model/mmoe.py:11-22) take any shape; a
 * refused one runs as the unfused composition in the host layer.
 * prepared (rs_mmoe_prepared_size floats, -1 on a bad shape), with dp =
 * roundup(d, 16), N1p = roundup((H + T) * E, 16), Kp_l / Np_l = roundup(
 * tower_dims[l] / tower_dims[l + 1], 16):
 *   dp * N1p + N1p + sum_l T * (Kp_l * Np_l + Np_l)
 * = [W1 | b1 | layer_0 .. layer_{L-1}]: W1 is ONE matrix [dp, N1p] in MFMA
 * B-fragment order whose column h * E + e is expert_matrix[:, h, e] (the Keras
 * tensor [d, H, E] read as [d, H * E]) and column H * E + t * E + e is
 * gate_matrix_t[:, e]; b1 the biases in the same column order; layer_l = the
 * T tasks' packed kernels [Kp_l, Np_l] one after another, then their T biases
 * [Np_l].  Padding is zeros.
 * rs_mmoe_prepare (mmoe_layer.build :438-477 + the towers' kernels): packs
 * it.  expert_matrix [d, H, E], expert_bias [H, E] (NULL =
 * use_expert_bias=False: zeros); gate_matrix / gate_bias: host arrays of T
 * device pointers ([d, E] / [E]; gate_bias, or any gate_bias[t], NULL =
 * zeros); tower_W / tower_bias: host arrays of T * n_tower_layers device
 * pointers, task-major (Keras kernels [in, out]; tower_bias, or any entry,
 * NULL = zeros).
 * rs_mmoe_fwd: mix (optional when n_tower_layers >= 1, required when 0 — the
 * launch is then mmoe_layer.call alone): [B, T * H], rows mix_stride apart,
 * task t at columns t * H.  y: task t's output [B, output_dim] at y + t *
 * y_task_stride, rows y_stride apart.  y is bit-identical with and without
 * mix, and mix with and without the towers.
 * Stream-ordered, graph-capturable; arguments are validated before any device
 * work; nothing is launched for batch 0.                                     */
int rs_mmoe_ok(int d, int hidden, int n_experts, int n_tasks,
               int n_tower_layers, const int* tower_dims);
int64_t rs_mmoe_prepared_size(int d, int hidden, int n_experts, int n_tasks,
                              int n_tower_layers, const int* tower_dims);
int rs_mmoe_prepare(int d, int hidden, int n_experts, int n_tasks,
                    const float* expert_matrix, const float* expert_bias,
                    const float* const* gate_matrix,
                    const float* const* gate_bias, int n_tower_layers,
                    const int* tower_dims, const float* const* tower_W,
                    const float* const* tower_bias, float* prepared,
                    rs_stream_t stream);
int rs_mmoe_fwd(const float* x, int64_t x_stride, int d, int hidden,
                int n_experts, int n_tasks, int n_tower_layers,
                const int* tower_dims, const int* tower_acts,
                const float* prepared, float* mix, int64_t mix_stride,
                float* y, int64_t y_task_stride, int64_t y_stride,
                int64_t batch, rs_stream_t stream);

/* Training MMOE (MMOE.train_step).  With L = n_tower_layers >= 1, n_l =
 * tower_dims[l + 1] (n_{L-1} = Nout), N1 = (H + T) * E:
 *   z_t = tower_t(mix_t) [B, Nout]                              (rs_mmoe_fwd)
 *   loss[t, b] = mean_j (max(z, 0) - z y + log1p(exp(-|z|)))   (the sigmoid
 *     cross-entropy of the towers' logits: BinaryCrossentropy(from_logits=
 *     True) per output, Keras' sum over the outputs weighted by loss_weights)
 *   G[b, t * Nout + j] = w_t * (sigmoid(z_t[b, j]) - y_t[b, j]) / (B * Nout)
 *   delta_{L-1} = G;  delta_{l-1} = (delta_l W_{t,l}^T) [a_{t,l-1} > 0] (no
 *     mask below a linear hidden layer);  dmix_t = delta_0 W_{t,0}^T
 *   dp_t[e] = sum_h dmix_t[h] expert[h, e]
 *   dlogit_t[e] = p_t[e] * (dp_t[e] - sum_e' p_t[e'] dp_t[e'])
 *   dexp[h, e] = [expert[h, e] > 0] * sum_t p_t[e] dmix_t[h]
 *   dz1 [B, N1]: column h * E + e = dexp[h, e], column H * E + t * E + e =
 *     dlogit_t[e] (the forward's stage-1 column order: x^T dz1 read as
 *     [d, H * E | T * E] is d expert_matrix [d, H, E], then the T gate
 *     matrices' gradients; its column sums are the bias gradients)
 *   dx = dz1 W1^T [B, d]
 * Every sum has one fixed order (h, e', t ascending), there are no atomics, a
 * row's result does not depend on the batch or on its place in its tile.
 * Masks are post-activation > 0 (rs_gemm's mask epilogue).  Hidden tower
 * activations: RS_ACT_RELU or RS_ACT_NONE; the output layer RS_ACT_NONE.
 * rs_mmoe_train_ok: 1 when the training entries take the shape: rs_mmoe_ok's
 * conditions, L >= 1, and the backward's three LDS tiles fit: with maxw =
 * max(roundup(d, 16), roundup(N1, 16), T * roundup(w, 16) over w in {H,
 * tower widths}), 4 * (48 * (roundup(maxw, 64) + 8) + 4096) <= 160 KiB.  It
 * never accepts a shape rs_mmoe_ok refuses.
 * saved (rs_mmoe_saved_size floats, -1 on a refused shape or batch < 0):
 *   B * (H * E + T * E + T * H + T * sum_{l < L-1} n_l)
 * = [expert [B, H * E] (column h * E + e, post-relu) | gates [B, T * E] |
 *    mix [B, T * H] | a_0 .. a_{L-2}, a_l [B, T * n_l] with task t at columns
 *    t * n_l], dense row-major.
 * rs_mmoe_train_fwd: rs_mmoe_fwd on the same `prepared` image, y
 * bit-identical, that also stores `saved`.
 * rs_mmoe_head_grad: the elementwise head.  z / labels: task t's [B, Nout]
 * at + t * task_stride, rows stride apart; loss_weights: HOST float[T] or
 * NULL (all 1); G [B, T * Nout], rows G_stride apart; loss [T, B] or NULL
 * (unweighted).
 * The backward image (rs_mmoe_bwd_prepared_size floats, -1 on a refused
 * shape; Kp_l / Np_l as above):
 *   sum_l T * Kp_l * Np_l + roundup(N1, 16) * roundup(d, 16)
 * = [chain layer L-1 .. 0 | W1^T]: chain layer l = the T tasks' W_{t,l}^T
 * ([Np_l, Kp_l]) in the forward's B-fragment layout one after another, no
 * biases; W1^T [roundup(N1, 16), roundup(d, 16)] with its rows in the
 * stage-1 column order.  rs_mmoe_prepare_bwd packs it (pointers as
 * rs_mmoe_prepare's).
 * rs_mmoe_bwd: ONE launch over 16-sample tiles for the whole data path.
 * deltas [B * T * sum_{l < L-1} n_l] has the layout of saved's a_l blocks
 * (delta_l = dL/d(pre-activation of hidden layer l); may be NULL when L = 1);
 * dz1 [B, N1], rows dz1_stride apart; dx [B, d], rows dx_stride apart, or
 * NULL = not computed (dz1 and deltas are bit-identical either way).  dmix,
 * dp and every other intermediate stay in LDS.
 * Stream-ordered, graph-capturable; arguments are validated before any device
 * work; nothing is launched for batch 0.                                     */
int rs_mmoe_train_ok(int d, int hidden, int n_experts, int n_tasks,
                     int n_tower_layers, const int* tower_dims);
int64_t rs_mmoe_saved_size(int d, int hidden, int n_experts, int n_tasks,
                           int n_tower_layers, const int* tower_dims,
                           int64_t batch);
int rs_mmoe_train_fwd(const float* x, int64_t x_stride, int d, int hidden,
                      int n_experts, int n_tasks, int n_tower_layers,
                      const int* tower_dims, const int* tower_acts,
                      const float* prepared, float* saved, float* y,
                      int64_t y_task_stride, int64_t y_stride, int64_t batch,
                      rs_stream_t stream);
int rs_mmoe_head_grad(const float* z, int64_t z_task_stride, int64_t z_stride,
                      const float* labels, int64_t labels_task_stride,
                      int64_t labels_stride, const float* loss_weights,
                      int n_out, int n_tasks, int64_t batch, float* G,
                      int64_t G_stride, float* loss, rs_stream_t stream);
int64_t rs_mmoe_bwd_prepared_size(int d, int hidden, int n_experts,
                                  int n_tasks, int n_tower_layers,
                                  const int* tower_dims);
int rs_mmoe_prepare_bwd(int d, int hidden, int n_experts, int n_tasks,
                        const float* expert_matrix,
                        const float* const* gate_matrix, int n_tower_layers,
                        const int* tower_dims, const float* const* tower_W,
                        float* prepared_bwd, rs_stream_t stream);
int rs_mmoe_bwd(const float* saved, const float* G, int64_t G_stride, int d,
                int hidden, int n_experts, int n_tasks, int n_tower_layers,
                const int* tower_dims, const int* tower_acts,
                const float* prepared_bwd, float* deltas, float* dz1,
                int64_t dz1_stride, float* dx, int64_t dx_stride,
                int64_t batch, rs_stream_t stream);

/* ------------------------------- DIEN interest evolution (a19), forward
 * model/dien.py:54-70 on a behaviour sequence keys [B, T, D], a candidate q
 * [B, D] and lengths len [B] (int32 or int64; position t is valid iff t <
 * len[b]: a length >= T makes every position valid, <= 0 none), in ONE launch
 * over 16-sample tiles:
 *   gru1 (Keras GRU, reset_after=True, gate order z r h; kernel W [D, 3 D],
 *   recurrent_kernel U [D, 3 D], bias [2, 3 D] = input row, recurrent row):
 *     xi = x_t W + bias[0]            hr = h U + bias[1]
 *     z = sig(xi_z + hr_z)  r = sig(xi_r + hr_r)  hh = tanh(xi_h + r * hr_h)
 *     h <- z * h + (1 - z) * hh       h_0 = 0, H1[b, t] = h
 *   scores (AttentionSequencePoolingLayer(return_score=True),
 *   layer/sequence.py:237-273, over LocalActivationUnit, layer/core.py:94-108):
 *     e_t = [q, H1_t, q - H1_t, q * H1_t]                       (4 D wide)
 *     y = act(act(e_t W_0 + b_0) W_1 + b_1)     s[b, t] = y . w_out + b_out
 *     weight_norm: s = -2^32 + 1 at t >= len, then softmax over T (the row
 *     maximum subtracted); else s = 0 at t >= len, no softmax
 *     att_act: RS_ACT_RELU, RS_ACT_SIGMOID or RS_ACT_DICE (inference Dice,
 *     layer/activation.py:32-66: p = sig((x - mean) / sqrt(var + 1e-9)),
 *     y = alpha * (1 - p) * x + p * x, per unit)
 *   gru2 (AUGRU over AUGRUCell, layer/sequence.py:293-395, layer/activation.py:
 *   91-142; no bias; hsig(x) = clip(0.2 x + 0.5, 0, 1); a = s[b, t]):
 *     z = a * hsig(x W_z + h U_z)     r = hsig(x W_r + h U_r)
 *     hh = tanh(x W_h + (r * h) U_h)
 *     h <- z * h + (1 - z) * hh       (augru_update 0, the reference)
 *     h <- (1 - z) * h + z * hh       (augru_update 1, the DIEN paper)
 *     x = H1_t, h_0 = 0, hist[b] = h after step T - 1
 * Both recurrences run all T steps, padded positions included (no Keras mask
 * reaches them: dien.py:116-117 builds the embeddings with
 * seq_mask_zero=False).
 * Layer 1 of the attention MLP is regrouped per sample as q (Wq + Wd) + b_0 +
 * H1_t (Wk - Wd) + (q * H1_t) Wp with W_0 = [Wq; Wk; Wd; Wp] (D rows each),
 * so its sums are ordered differently from e_t W_0 (fp32 rounding only).
 * A sample's results do not depend on the batch, its tile mates or the
 * optional outputs: hist is bit-identical with and without H1 / scores, for
 * any split of the batch, and between the dense and the ids form.
 * Caps of the one-launch form (rs_dien_evolution_ok: 1 when it takes the
 * shape): 1 <= D <= 64; exactly two attention layers, each 1..128 wide;
 * att_act one of the three; and, with Dp = roundup(D, 16), the tile's LDS
 *   4 * (16 * T * Dp + 32 * Dp + 16 * T) <= 160 KiB
 * (the sequence tile that becomes H1, the state and r * h tiles, the scores) —
 * T <= 50 at D 36, T <= 148 at D <= 16.  A refused shape runs unfused in the
 * host layer (rs_gru_fwd, the scores from older entries / torch,
 * rs_augru_fwd).  H1 is not spilled to a global workspace for larger T: the
 * unfused path already keeps H1 in HBM, and a third variant would only
 * duplicate it.
 * prepared (rs_dien_prepared_size floats, -1 on a bad shape; independent of
 * T), with A1p / A2p = roundup(att_hidden[0] / [1], 16):
 *   2 * (6 * Dp * Dp + 6 * Dp)                       the two gru images
 *   + 3 * A1p * Dp + 4 * A1p + A2p * A1p + 5 * A2p + 4   the attention image
 * gru image (rs_gru_prepared_size(din, units) = 3 * Up * Kp + 3 * Up * Up +
 * 6 * Up floats, Kp / Up = roundup(din / units, 16); din, units <= 64): [W | U
 * | bias [2][3][Up]], a matrix as 3 gates x Up / 16 column tiles x k-groups of
 * MFMA fragments (lane l, element j: M[16 g + 4 (l >> 4) + j][gate * units +
 * 16 c + (l & 15)]); attention image: [Wk - Wd | Wp | Wq + Wd | b_0 | dice_0
 * (mean, 1 / sqrt(var + 1e-9), alpha) | W_1 | b_1 | dice_1 | w_out | b_out
 * (4)], matrices in the same fragment order.  Padding is zeros.
 * rs_dien_prepare: att_W / att_b / dice_*: host arrays of n_att_layers device
 * pointers (Keras kernels [in, out]; dice_* read for RS_ACT_DICE only, else
 * may be NULL); gru1_bias [2, 3 D]; att_out_w [att_hidden[1]], att_out_b [1].
 * rs_gru_prepare: bias NULL = zeros (the AUGRU has none).
 * rs_dien_evolution_fwd: keys[b, t, :] at keys + b * keys_bstride + t *
 * keys_tstride; optional H1 [B, T, D] and scores [B, T] (contiguous); hist
 * [B, D], rows hist_stride apart.
 * rs_dien_evolution_ids_fwd: 1..4 behaviour features concatenated along D
 * (widths add up to D): feature f's history ids hist_ids[f] [B, T] (rows
 * hist_strides[f] elements apart), candidate ids cand_ids[f] [B] (cand_strides
 * [f] apart), both of kinds[f] (RS_ID_*), looked up in tables[f] [vocabs[f],
 * widths[f]].  An id outside [0, vocab) reads a zero row and sets *err_flag.
 * The [B, T, D] keys are never written to HBM.
 * rs_gru_fwd (x [B, T, din] -> seq [B, T, units] and / or last [B, units]) and
 * rs_augru_fwd (x, scores [B, T] -> last) are the same device functions as
 * stand-alone launches, reading x step by step from global memory; din may
 * differ from units.
 * Stream-ordered, graph-capturable; arguments are validated before any device
 * work; nothing is launched for batch 0.                                     */
#define RS_ACT_DICE 4 /* rs_dien_* only */
int rs_dien_evolution_ok(int T, int D, int n_att_layers, const int* att_hidden,
                         int att_act);
int64_t rs_dien_prepared_size(int D, int n_att_layers, const int* att_hidden);
int rs_dien_prepare(int D, const float* gru1_kernel,
                    const float* gru1_recurrent, const float* gru1_bias,
                    const float* gru2_kernel, const float* gru2_recurrent,
                    int n_att_layers, const int* att_hidden, int att_act,
                    const float* const* att_W, const float* const* att_b,
                    const float* const* dice_mean,
                    const float* const* dice_var,
                    const float* const* dice_alpha, const float* att_out_w,
                    const float* att_out_b, float* prepared,
                    rs_stream_t stream);
int rs_dien_evolution_fwd(const float* keys, int64_t keys_bstride,
                          int64_t keys_tstride, const float* q,
                          int64_t q_stride, const void* len, int len_kind,
                          int T, int D, int n_att_layers,
                          const int* att_hidden, int att_act, int weight_norm,
                          int augru_update, const float* prepared, float* H1,
                          float* scores, float* hist, int64_t hist_stride,
                          int64_t batch, rs_stream_t stream);
int rs_dien_evolution_ids_fwd(int n_feat, const int* widths, const int* kinds,
                              const void* const* hist_ids,
                              const int64_t* hist_strides,
                              const void* const* cand_ids,
                              const int64_t* cand_strides,
                              const float* const* tables,
                              const int64_t* vocabs, const void* len,
                              int len_kind, int T, int D, int n_att_layers,
                              const int* att_hidden, int att_act,
                              int weight_norm, int augru_update,
                              const float* prepared, float* H1, float* scores,
                              float* hist, int64_t hist_stride, int64_t batch,
                              int* err_flag, rs_stream_t stream);
int64_t rs_gru_prepared_size(int din, int units);
int rs_gru_prepare(int din, int units, const float* kernel,
                   const float* recurrent, const float* bias, float* prepared,
                   rs_stream_t stream);
int rs_gru_fwd(const float* x, int64_t x_bstride, int64_t x_tstride, int T,
               int din, int units, const float* prepared, float* seq,
               float* last, int64_t last_stride, int64_t batch,
               rs_stream_t stream);
int rs_augru_fwd(const float* x, int64_t x_bstride, int64_t x_tstride,
                 const float* scores, int64_t scores_stride, int T, int din,
                 int units, int augru_update, const float* prepared,
                 float* last, int64_t last_stride, int64_t batch,
                 rs_stream_t stream);

/* ------------------------- training of DIEN's recurrences (dien_train.hip)
 * Backpropagation through time of the GRU and the AUGRU above, gate order
 * z r h.  Steps run t = T-1 .. 0, padded positions included; dh is the
 * upstream gradient of h_t: dseq[b, t] where given, plus dlast at t = T-1,
 * plus the carry from step t + 1.
 * GRU, a_z = xi_z + hr_z, a_r = xi_r + hr_r, c = xi_h + r hr_h:
 *   dz = dh (h_prev - hh)   dhh = dh (1 - z)   dc = dhh (1 - hh^2)
 *   da_z = dz z (1 - z)     dr = dc hr_h       da_r = dr r (1 - r)
 *   gx = [da_z, da_r, dc]   gh = [da_z, da_r, dc r]   carry = dh z + gh U^T
 * AUGRU, u = hsig(a_z), z = a u, r = hsig(a_r), a = scores[b, t]:
 *   reference blend: dz = dh (h_prev - hh), keep = dh z,       dhh = dh (1 - z)
 *   paper blend:     dz = dh (hh - h_prev), keep = dh (1 - z), dhh = dh z
 *   dc = dhh (1 - hh^2)   d(rh) = dc U_h^T   dr = d(rh) h_prev
 *   da[b, t] = sum_units dz u   da_z = dz a hsig'(a_z)   da_r = dr hsig'(a_r)
 *   (hsig' = 0.2 where 0 < hsig < 1, else 0)   gx = [da_z, da_r, dc]
 *   carry = keep + d(rh) r + [da_z, da_r] U_zr^T
 * rs_gru_train_fwd / rs_augru_train_fwd: rs_gru_fwd / rs_augru_fwd (the same
 * device functions: seq / last are bit-identical to theirs) that also write
 * `saved`, rs_gru_saved_size / rs_augru_saved_size(T, din, units, batch) =
 * batch * T * 5 * Up / batch * T * 4 * Up floats (Up = roundup(units, 16);
 * -1 on a bad shape): per (b, t) the planes z | r | hh | hr_h | h_prev (GRU)
 * or u | r | hh | h_prev (AUGRU), Up floats each.  saved is 16-byte aligned.
 * As in rs_gru_fwd, at least one of seq / last is required.
 * rs_gru_prepare_bwd: the transposed recurrent kernel [units, 3 units] as MFMA
 * fragments (rs_gru_bwd_prepared_size(units) = 3 * Up * Up floats: gate, unit
 * tile c, k-group g, lane l, element j = U[16 c + (l & 15)][gate * units + 16 g
 * + 4 (l >> 4) + j], zero padded); one image serves both recurrences.
 * rs_gru_bwd (dseq [B, T, units] contiguous and / or dlast [B, units], rows
 * dlast_stride apart; one of them may be NULL) and rs_augru_bwd (dlast
 * required) are one launch over 16-sample tiles with only the h -> h chain in
 * the time loop.  They write the operands of everything off the chain as
 * contiguous matrices of B * T rows (row b * T + t):
 *   gx [B T, 3 units]; GRU: gh [B T, 3 units] and hprev [B T, units] (row t =
 *   0 is zeros); AUGRU: hrh [B T, 2 units] = [h_prev | r h_prev]
 * so that with x as [B T, din]
 *   dx = gx W^T, dW = x^T gx, GRU: dU = hprev^T gh, dbias = [colsum gx; colsum
 *   gh]; AUGRU: dU[:, :2 units] = h_prev^T gx[:, :2 units], dU[:, 2 units:] =
 *   (r h_prev)^T gx[:, 2 units:]
 * are rs_gemm / rs_col_sum_split calls.  rs_augru_bwd also returns the
 * gradient of the scores through the forward's mask (scores: the forward's
 * output, rows scores_stride apart; len, weight_norm as in the forward):
 *   weight_norm: ds_t = p_t (da_t - sum_{tau < len} p_tau da_tau) for t < len
 *   else:        ds_t = da_t for t < len;   exactly 0 for t >= len
 * (a row with len <= 0 is all zeros), and the raw da [B, T] where da is not
 * NULL.  Caps: units <= 64 (din <= 64 in the forwards); no cap on T: saved
 * state and upstream gradients are read step by step from global memory.
 * Deterministic; the per-sample results (gx, gh, hprev, hrh, ds, da) do not
 * depend on the batch or its tile mates, and neither does dx = gx W^T when
 * its rs_gemm is called without a workspace (one pass over K = 3 units; with
 * one, the number of K slices follows the batch).  Stream-ordered,
 * graph-capturable; arguments are validated before any device work; nothing
 * is launched for batch 0; every element of every output is written.       */
int64_t rs_gru_saved_size(int T, int din, int units, int64_t batch);
int64_t rs_augru_saved_size(int T, int din, int units, int64_t batch);
int64_t rs_gru_bwd_prepared_size(int units);
int rs_gru_prepare_bwd(int units, const float* recurrent, float* prepared_bwd,
                       rs_stream_t stream);
int rs_gru_train_fwd(const float* x, int64_t x_bstride, int64_t x_tstride,
                     int T, int din, int units, const float* prepared,
                     float* seq, float* last, int64_t last_stride,
                     float* saved, int64_t batch, rs_stream_t stream);
int rs_augru_train_fwd(const float* x, int64_t x_bstride, int64_t x_tstride,
                       const float* scores, int64_t scores_stride, int T,
                       int din, int units, int augru_update,
                       const float* prepared, float* last,
                       int64_t last_stride, float* saved, int64_t batch,
                       rs_stream_t stream);
int rs_gru_bwd(const float* saved, const float* dseq, const float* dlast,
               int64_t dlast_stride, int T, int units,
               const float* prepared_bwd, float* gx, float* gh, float* hprev,
               int64_t batch, rs_stream_t stream);
int rs_augru_bwd(const float* saved, const float* scores,
                 int64_t scores_stride, const void* len, int len_kind,
                 int weight_norm, const float* dlast, int64_t dlast_stride,
                 int T, int units, int augru_update,
                 const float* prepared_bwd, float* gx, float* hrh, float* ds,
                 float* da, int64_t batch, rs_stream_t stream);

/* ------------------------------------- DSSM two-tower retrieval (a20), forward
 * model/dssm.py:17-90: a user tower and an item tower, each
 *   [SparseFeat rows | pooled var-len features | dense values]  ->  DNN  ->
 *   tf.math.l2_normalize(axis=-1)
 * (layer/utils.py:140-150, utils/inputs.py:142-153), then the in-batch
 * sampled-softmax loss (layer/activation.py:267-285, layer/utils.py:206-215)
 * or the 'logistic' score.
 *
 * rs_seq_pool_fwd: SequencePoolingLayer (layer/sequence.py:20-95), 1..8
 * features per launch.  Feature f pools T = Ts[f] positions of widths[f] = E
 * columns into out[b * out_stride + out_cols[f] ..]; combiners[f] = 0 sum,
 * 1 mean, 2 max.  Source: kinds[f] = RS_ID_*: ids srcs[f] [B, T] (rows
 * src_strides[f] elements apart) looked up in tables[f] [vocabs[f], E] (an id
 * outside [0, vocab) at a valid position reads a zero row and sets
 * *err_flag); kinds[f] = -1: embedded values srcs[f] [B, T, E] fp32 (samples
 * src_strides[f] floats apart), the layer's own call.  Mask: lengths[f] [B]
 * (len_kinds[f] = RS_ID_I32 / RS_ID_I64; position t valid iff t < len, the
 * supports_masking=False form) or, with lengths[f] NULL (lengths itself may be
 * NULL), the supports_masking=True form: an id source's mask is id != 0 (Keras
 * mask_zero), a dense source's is masks[f] (uint8 [B, T], non-zero = valid),
 * and the length is the number of valid positions.
 *   sum  = the valid rows added;  mean = sum / (float(len) + 1e-8) — a length
 *   above T keeps all T positions and divides by the length given, a length
 *   <= 0 gives 0;  max = max of x - (1 - mask) * 1e9: masked rows are skipped
 *   and stand as -1e9, exact while |x| < 32 (beyond that the reference's
 *   x - 1e9 keeps some of x's bits; a documented deviation).
 * One wave per (sample, feature).  A row is read by E / 4 lanes (float4; E
 * lanes when 4 does not divide E or the rows are not 16-byte aligned), so the
 * wave holds G = min(64 / lanes-per-row, 16) rows at once.  Sum order, fixed
 * per sample and independent of the batch: lane group g adds positions t = g,
 * g + G, g + 2 G, ... ascending, starting from 0; the G partial rows are then
 * added in group order, ((p_0 + p_1) + p_2) + ...  The rows of masked
 * positions are not loaded (the ids of all T positions are).  Caps: E <= 64,
 * or a multiple of 4 up to 256.
 *
 * rs_dssm_tower_fwd: one tower in one launch over 16-sample tiles.  The
 * single-id and dense pieces are rs_concat_pieces' (n_pieces, widths, in_cols
 * = first input column, kinds, srcs, src_strides, tables, vocabs), the
 * sequence pieces rs_seq_pool_fwd's (n_seq, seq_*, combiners, lengths,
 * len_kinds, masks); together 1..16 pieces that tile the dims[0] input columns
 * exactly.  The row is staged in LDS, runs the n_layers Dense layers of
 * `prepared` (rs_mlp_prepare on dims / the layers' kernels; acts[l] NONE /
 * RELU / SIGMOID) and is normalised: out[b, :dims[n_layers]] = x *
 * rsqrt(max(sum x^2, 1e-12)).  n_layers = 0 (an empty item_dnn_hidden_units,
 * model/dssm.py:68-70) normalises the staged row (prepared may be NULL).
 * Neither the concat nor an activation reaches HBM.  out is bit-identical to
 * rs_concat_pieces + rs_seq_pool_fwd into a [B, dims[0]] buffer, rs_mlp_fwd
 * (head 0), rs_l2_normalize_fwd — the same device functions — for any split
 * of the batch.  rs_dssm_tower_ok(n_pieces + n_seq, n_layers, dims, acts): 1
 * when the one-launch form takes the shape: 1..16 pieces, 0..8 layers, every
 * width 1..1024, the rs_mlp_fwd tile within 160 KiB of LDS
 * (rs_mlp_prepared_size >= 0), activations NONE / RELU / SIGMOID (a
 * BatchNormalization, Dice or PReLU tower runs unfused in the host layer), and
 * not the 256 -> 128 -> 64 -> 1 shape rs_mlp_fwd runs as its split-K tail.
 * rs_l2_normalize_fwd: y[m, :N] = x[m] * rsqrt(max(sum_n x[m, n]^2, 1e-12)),
 * one wave per row: lane l adds columns l, l + 64, ... ascending (fma), then a
 * fixed butterfly over the wave.  In place allowed.
 *
 * rs_inbatch_softmax_fwd: user [B, E], item [B, E] (rows *_stride apart),
 * item_idx [B] (RS_ID_I32 / RS_ID_I64), logq [n_items] = log(item_count /
 * sum(item_count)):
 *   z_ij = (u_i / temperature) . v_j - logq[item_idx[j]]
 *   loss[i] = logsumexp_j z_ij - z_ii
 * A workgroup owns 16 user rows; its 16 waves walk the item column tiles
 * (wave w: tiles w, w + 16, ...) with v_mfma_f32_16x16x4_f32, K = E zero-padded
 * to a multiple of 16, and keep a running (max, sum) per row; the partials
 * merge in a fixed order (the 16 lanes of a row, then the waves in wave
 * order), so the loss is bit-reproducible from run to run.  No [B, B] buffer
 * and no workspace.  Columns past B are excluded; duplicated items are not
 * masked (as the reference); an item_idx outside [0, n_items) uses logq = 0
 * and sets *err_flag.  rs_inbatch_softmax_ok(E): 1 for 1 <= E <= 512.
 * rs_dssm_score_fwd: out[b] = sigmoid((sum_k u_bk v_bk) / temperature), the
 * 'logistic' head reduced over the last axis (the reference's
 * tf.reduce_sum has no axis).
 * All entries: stream-ordered, graph-capturable, no allocation; arguments are
 * validated before any device work; nothing is launched for batch 0; every
 * loop is bounded by an argument.                                           */
int rs_seq_pool_fwd(int n_feat, const int* widths, const int* out_cols,
                    const int* Ts, const int* combiners, const int* kinds,
                    const void* const* srcs, const int64_t* src_strides,
                    const float* const* tables, const int64_t* vocabs,
                    const void* const* lengths, const int* len_kinds,
                    const void* const* masks, float* out, int64_t out_stride,
                    int64_t batch, int* err_flag, rs_stream_t stream);
int rs_l2_normalize_fwd(const float* x, int64_t x_stride, float* y,
                        int64_t y_stride, int64_t M, int N, rs_stream_t stream);
int rs_dssm_tower_ok(int n_pieces, int n_layers, const int* dims,
                     const int* acts);
int rs_dssm_tower_fwd(int n_pieces, const int* widths, const int* in_cols,
                      const int* kinds, const void* const* srcs,
                      const int64_t* src_strides, const float* const* tables,
                      const int64_t* vocabs, int n_seq, const int* seq_widths,
                      const int* seq_cols, const int* seq_Ts,
                      const int* combiners, const int* seq_kinds,
                      const void* const* seq_srcs, const int64_t* seq_strides,
                      const float* const* seq_tables,
                      const int64_t* seq_vocabs, const void* const* lengths,
                      const int* len_kinds, const void* const* masks,
                      int n_layers, const int* dims, const int* acts,
                      const float* prepared, float* out, int64_t out_stride,
                      int64_t batch, int* err_flag, rs_stream_t stream);
int rs_inbatch_softmax_ok(int E);
int rs_inbatch_softmax_fwd(const float* user, int64_t user_stride,
                           const float* item, int64_t item_stride,
                           const void* item_idx, int idx_kind,
                           const float* logq, int64_t n_items,
                           float temperature, float* loss, int64_t batch, int E,
                           int* err_flag, rs_stream_t stream);
int rs_dssm_score_fwd(const float* user, int64_t user_stride,
                      const float* item, int64_t item_stride,
                      float temperature, float* out, int64_t batch, int E,
                      rs_stream_t stream);

/* ------------------------------------------------- DSSM training (a31)
 * One step of Keras fit on model/dssm.py:149-152 (optimizer "adam", loss
 * sampledsoftmaxloss = the batch mean of the in-batch softmax losses).
 *
 * rs_inbatch_softmax_train_fwd: rs_inbatch_softmax_fwd that also writes
 * lse[i] = logsumexp_j z_ij.  The same device function walks the tiles, so
 * loss is bit-identical to rs_inbatch_softmax_fwd's.
 *
 * rs_inbatch_softmax_bwd: with p_ij = exp(z_ij - lse_i) and
 * dz_ij = g_i (p_ij - [i == j]) (g = NULL: g_i = 1 / B; logq is a constant;
 * duplicated items are not masked),
 *   du[i] = (1 / temperature) sum_j dz_ij v_j
 *   dv[j] = sum_i dz_ij (u_i / temperature)
 * Two launches of one kernel.  A workgroup owns 16 user rows (du) or 16 item
 * rows (dv); its 8 waves walk the other side's 16-row tiles (wave w: tiles w,
 * w + 8, ...): the logits tile is recomputed with v_mfma_f32_16x16x4_f32 with
 * the OTHER side on the accumulator's rows (du recomputes z^T, dv z), dz is
 * formed in those registers and is the B operand of the second MFMA product
 * as it stands; K = E zero-padded to a multiple of 16.  Sum order: within a
 * wave its tiles ascending (inside a tile the MFMA's k order), then the
 * waves' partial tiles in wave order — no [B, B] buffer, no atomics, du and dv
 * bit-identical from run to run.  An item_idx outside [0, n_items) uses
 * logq = 0 and sets *err_flag.  rs_inbatch_softmax_bwd_ok(E): 1 for
 * 1 <= E <= 256 (nine 16-row tiles of E + 4 floats in the 160 KiB of LDS;
 * the E / 4 accumulator registers per lane would allow 512).
 *
 * rs_l2_normalize_bwd: for y = x r, r = rsqrt(max(s, 1e-12)), s = sum x^2:
 * dx = r (dy - y (y . dy)) where s >= 1e-12, r dy (= 1e6 dy) below.  One wave
 * per row; s and y . dy are the forward's sums: lane l adds columns l, l + 64,
 * ... ascending (fma), then the fixed butterfly.  dx may alias dy.
 *
 * rs_embedding_grad_accum: G[id(b, t), 0:k] += scale_b grad[b, 0:k] for every
 * valid position of ids [B, T] (rows id_stride apart), G dense [n_rows, k].
 * combiner -1: every position is valid and scale_b = 1 (T = 1: a SparseFeat
 * column); 0 (sum) / 1 (mean): rs_seq_pool_fwd's validity — t < lengths[b]
 * (int32 / int64; a length above T keeps all T, <= 0 none) or, with lengths
 * NULL, id != 0 — and scale_b = 1 or 1 / (float(len_b) + 1e-8), len_b the
 * length input or the count of non-zero ids, computed on the device.  The
 * lookups are sorted by row (stable radix sort), a row's duplicates are summed
 * in lookup order (b, t) ascending (chunked segment sums, as
 * rs_embedding_sgd_strided) and added to G once; the gradient row is read
 * through the sorted position, so no [B, T, k] buffer exists.  An id outside
 * [0, n_rows) at a valid position sets *err_flag and contributes nothing.
 * workspace: rs_embedding_grad_accum_workspace_size(batch * T) bytes.
 *
 * rs_adam_update_multi: Keras optimizer_v2 Adam over count tensors, 32 per
 * launch: with t = *step + 1 (step: int64 in device memory, so a captured
 * step replays correctly), g = grad + 2 l2 w,
 *   lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t)   (float; 1 - beta^t as
 *                                        -expm1(t log beta))
 *   m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2
 *   w -= lr_t m / (sqrt(v) + eps)
 * beta1 / beta2 are the float32 values Keras' own variables hold; 1 - beta and
 * log beta are formed from them in double and rounded once.  rs_adam_advance: *step += 1 on the stream (after the last
 * rs_adam_update_multi of the step).
 * All entries: stream-ordered, graph-capturable, no allocation; arguments are
 * validated before any device work; nothing is launched for batch 0; every
 * loop is bounded by an argument.                                           */
int rs_inbatch_softmax_train_fwd(const float* user, int64_t user_stride,
                                 const float* item, int64_t item_stride,
                                 const void* item_idx, int idx_kind,
                                 const float* logq, int64_t n_items,
                                 float temperature, float* loss, float* lse,
                                 int64_t batch, int E, int* err_flag,
                                 rs_stream_t stream);
int rs_inbatch_softmax_bwd_ok(int E);
int rs_inbatch_softmax_bwd(const float* user, int64_t user_stride,
                           const float* item, int64_t item_stride,
                           const void* item_idx, int idx_kind,
                           const float* logq, int64_t n_items,
                           float temperature, const float* lse, const float* g,
                           float* du, int64_t du_stride, float* dv,
                           int64_t dv_stride, int64_t batch, int E,
                           int* err_flag, rs_stream_t stream);
int rs_l2_normalize_bwd(const float* x, int64_t x_stride, const float* dy,
                        int64_t dy_stride, float* dx, int64_t dx_stride,
                        int64_t M, int N, rs_stream_t stream);
int64_t rs_embedding_grad_accum_workspace_size(int64_t n_lookups);
int rs_embedding_grad_accum(float* G, int64_t n_rows, int k, const void* ids,
                            int id_kind, int64_t id_stride, int T,
                            const void* lengths, int len_kind, int combiner,
                            const float* grad, int64_t grad_stride,
                            int64_t batch, void* workspace, int* err_flag,
                            rs_stream_t stream);
int rs_adam_update_multi(int count, float* const* w, const float* const* grad,
                         float* const* m, float* const* v, const int64_t* n,
                         const float* l2, float lr, float beta1, float beta2,
                         float eps, const int64_t* step, rs_stream_t stream);
int rs_adam_advance(int64_t* step, rs_stream_t stream);

/* ----------------------------------------------- DSSM retrieval (a20)
 * rs_topn_inner_product: exact top-N by inner product.  user [U, E], item
 * [I, E] (rows *_stride apart); for every user row u the N items with the
 * largest score(u, i) = sum_k user[u, k] item[i, k], ordered by the key
 * (score descending, item position ascending): out_idx [U, N] the positions
 * into item, out_score [U, N] the scores, both contiguous.  A tie in score
 * goes to the lower position.  Where I < N the slots past I hold position -1
 * and score -inf (I = 0: every slot).
 *
 * Two kernels (csrc/topn.hip).  The partial kernel runs on a grid of (64-row
 * user tiles) x (item splits): the user tile in LDS, 8 waves walking the
 * split's 16-item tiles with v_mfma_f32_16x16x4_f32 (an item tile's operand
 * loaded once and used by the four 16-row blocks), a sorted best-N list and a
 * 32-entry candidate queue per row in LDS; a score enters the queue only if
 * it beats the row's N-th key.  The merge kernel (one workgroup per user)
 * merges the splits' sorted lists from the workspace pairwise in LDS; with one
 * split the partial kernel writes the result itself.  A score is one MFMA
 * chain per pair, the same bits wherever the pair falls, and every comparison
 * is on the 64-bit key (score, ~position), so the output is bit-identical for
 * every item_splits.  item_splits 0: chosen from U and I (two workgroups per
 * CU, at least 64 tiles per split); otherwise clamped to 1..64 and to the
 * number of 16-item tiles.  No [U, I] buffer, no global atomics; the
 * workspace (rs_topn_inner_product_workspace_size bytes for the same U, I, N,
 * item_splits; 0 with one split in effect; 8-byte aligned) need not be
 * zeroed.  Item rows that are not 16-byte aligned, or E % 4 != 0, are loaded
 * by scalars.  Inputs are taken as finite: a NaN score gets some rank and
 * breaks nothing.  rs_topn_inner_product_ok(E, N): 1 for 1 <= E <= 512,
 * 1 <= N <= 128 and 64 (rup(E, 64) + 8) 4 + 64 (N + 32) 8 + 784 bytes of LDS
 * within 160 KiB — every (E <= 256, N <= 128); E = 512 up to N = 26.  A
 * refused shape is RS_ERR_ARG.  I < 2^31.  Stream-ordered, graph-capturable,
 * no allocation, no host synchronisation; nothing is launched for U = 0.    */
int rs_topn_inner_product_ok(int E, int N);
int64_t rs_topn_inner_product_workspace_size(int64_t U, int64_t I, int N,
                                             int item_splits);
int rs_topn_inner_product(const float* user, int64_t user_stride, int64_t U,
                          const float* item, int64_t item_stride, int64_t I,
                          int E, int N, int item_splits /* 0 = auto */,
                          int32_t* out_idx /* [U, N] */,
                          float* out_score /* [U, N] */, void* workspace,
                          int64_t workspace_bytes, rs_stream_t stream);

/* ------------------------------------------ wide part of Wide&Deep (a17)
 * WideLayer.call (layer/interaction.py:11-26: w0 + x @ w) on the compact form
 * of WideDeep's wide input (model/wideDeep.py:22-34): x = [dense (nd) | dense
 * again (nd) | one-hot], one 1 per field at column 2 nd + field_offsets[c] +
 * id(b, c):
 *   logit[b] = w0 + sum_j dense[b,j] (w[j] + w[nd+j]) + sum_c w[2 nd + off_c + id_c]
 * summed in that order.  field_widths[c] = the field's one-hot width; a code
 * outside [0, width_c) contributes 0 and sets *err_flag.  w [2 nd + sum of
 * the widths], w0 [1].  No one-hot matrix is formed.                        */
int rs_wide_onehot_fwd(const void* ids, int id_kind, int64_t id_stride,
                       const float* dense, int64_t dense_stride, int nd,
                       const int64_t* field_offsets,
                       const int64_t* field_widths, int n_fields,
                       const float* w, const float* w0, float* logit,
                       int64_t batch, int* err_flag, rs_stream_t stream);

/* --------------------------------------------- fused DeepFM forward (a8)
 * DeepFM.call (model/deepFM.py:23-31) in ONE launch: ids -> rows -> x (kept
 * in LDS) -> FM logit and the DNN tower -> out[b] = sigmoid(c0*dnn + c1*fm)
 * (reference: c0 = c1 = 0.5).  Arguments as rs_embed_fm_fwd plus the tower
 * (rs_mlp_*).  mlp_prepared must be packed with in_rows mapping the LDS
 * column order [emb F*k | dense nd] to Keras rows: p < F*k -> nd + p,
 * F*k <= p < F*k+nd -> p - F*k, else -1.  fm_logit (optional) receives the
 * FM logit.  rs_deepfm_fused_ok: 1 when the shape is supported (k 8 or 16,
 * kfm <= 15, 1..128 fields, tower output 1, dims[0] = nd + F*k).            */
int rs_deepfm_fused_ok(int nd, int n_fields, int k, int kfm, int n_layers,
                       const int* dims);
int rs_deepfm_fwd(const void* ids, int id_kind, int64_t id_stride,
                  const float* dense, int64_t dense_stride, int nd,
                  const float* table, const int64_t* field_offsets,
                  const int64_t* field_vocab, int n_fields, int k,
                  const float* fm_prepared, const float* w0, int kfm,
                  int n_layers, const int* dims, const int* acts,
                  const float* mlp_prepared, float c0, float c1, float* out,
                  float* fm_logit, int64_t batch, int* err_flag,
                  rs_stream_t stream);
/* rs_deepfm_fwd with the field metadata also on the host (kernel arguments
 * for n_fields <= 32, as rs_embed_fm_fwd_hm; the host arrays must equal the
 * device ones).                                                             */
int rs_deepfm_fwd_hm(const void* ids, int id_kind, int64_t id_stride,
                     const float* dense, int64_t dense_stride, int nd,
                     const float* table, const int64_t* field_offsets,
                     const int64_t* field_vocab,
                     const int64_t* field_offsets_host,
                     const int64_t* field_vocab_host, int n_fields, int k,
                     const float* fm_prepared, const float* w0, int kfm,
                     int n_layers, const int* dims, const int* acts,
                     const float* mlp_prepared, float c0, float c1, float* out,
                     float* fm_logit, int64_t batch, int* err_flag,
                     rs_stream_t stream);

/* Dense + PReLU whose alpha is [alpha_rows, N], row m using alpha row
 * m % alpha_rows: Keras Dense(N, activation=PReLU()) on a 3-D input
 * [B, alpha_rows, K] flattened to [B*alpha_rows, K] (PReLU's alpha has shape
 * input_shape[1:] = (T, N)).                                                */
int rs_dense_prelu_rows_fwd(const float* x, int64_t x_stride, const float* W,
                            const float* bias, const float* alpha,
                            int alpha_rows, float* y, int64_t y_stride,
                            int64_t M, int K, int N, rs_stream_t stream);

/* Per-column affine + activation, in place allowed: y = act(x*scale + shift).
 * Used for BatchNormalization at inference (model/din.py:89).               */
int rs_affine_act(const float* x, int64_t x_stride, const float* scale,
                  const float* shift, const float* alpha, int act, float* y,
                  int64_t y_stride, int64_t M, int N, rs_stream_t stream);

/* Dice at inference on a 2-D input (layer/interaction.py:410-425), per column
 * n: xhat = (x-mean[n])/sqrt(var[n]+eps), p = sigmoid(xhat),
 *    y = alpha[n]*(1-p)*x + p*x.  Used for DIN's dnn_activation='dice'.     */
int rs_dice_fwd(const float* x, int64_t x_stride, const float* mean,
                const float* var, float eps, const float* alpha, float* y,
                int64_t y_stride, int64_t M, int N, rs_stream_t stream);

/* Model heads: out[b] = sigmoid(c0*a[b] + c1*b[b]) (b may be NULL).
 * DeepFM: sigmoid(0.5*(fm+dnn)) (model/deepFM.py:30).                       */
int rs_sigmoid_combine(const float* a, const float* b, float c0, float c1,
                       float* out, int64_t n, rs_stream_t stream);

/* ------------------------- other interactions on the gather (§8(f) rank 3)
 * rs_embed_pair_pool_fwd: per sample, the F field rows e_c (one concatenated
 *  table, per-field offsets) pooled over the P = F(F-1)/2 pair products
 *  e_i*e_j (per dim): mode 0 = sum = 0.5((sum e)^2 - sum e^2) — NFM's
 *  bi-interaction (model/nfm.py:28) and AFM 'att' (AttentionLayer's softmax
 *  over a size-1 axis is 1, layer/interaction.py:313-318); mode 1 = mean
 *  (AFM 'avg'); mode 2 = max (AFM 'max', F <= 64).  Outputs (any subset):
 *  out[b*out_stride + out_col + j] = pooled_j and out[b*out_stride + i] =
 *  dense[b, i] for i < nd (NFM's concat([dense, emb]), model/nfm.py:29);
 *  head_out[b] = sigmoid^n_sigmoid(pooled @ head_w + head_b) (AFMLayer's
 *  Dense(1) + sigmoid, then AFM.call's second sigmoid: n_sigmoid = 2).
 * rs_pair_products_fwd: InteractionLayer (layer/interaction.py:280-297):
 *  e [batch, F*k] (row stride e_stride) -> out [batch, P, k], pairs i<j
 *  row-major.
 * rs_ffm_fwd: FFMLayer.call + FFM.call (layer/interaction.py:134-163,
 *  model/ffm.py:20-22) on label-encoded ids: x = [dense | one-hot], feature
 *  f = nd + field_offsets[c] + id; v [feature_num, (nd+F)*k], w
 *  [feature_num]; out[b] = sigmoid^n_sigmoid(w0 + x@w + sum_{f<g}
 *  <field_f, field_g>), field = x @ v; k divides 64, (nd+F)*k <= 1024.      */
int rs_embed_pair_pool_fwd(const void* ids, int id_kind, int64_t id_stride,
                           const float* table, const int64_t* field_offsets,
                           const int64_t* field_vocab, int n_fields, int k,
                           int mode, const float* dense, int64_t dense_stride,
                           int nd, float* out, int64_t out_stride, int out_col,
                           const float* head_w, const float* head_b,
                           int n_sigmoid, float* head_out, int64_t batch,
                           int* err_flag, rs_stream_t stream);
int rs_pair_products_fwd(const float* e, int64_t e_stride, int n_fields, int k,
                         int64_t batch, float* out, rs_stream_t stream);
/* AttentionLayer.call (layer/interaction.py:310-319) on x [batch, n_rows, k]
 * (row stride x_stride): its softmax runs over a size-1 axis (every score is
 * exactly 1), so out[b, j] = sum_p x[b, p, j].                             */
int rs_attention_pool_fwd(const float* x, int64_t x_stride, int n_rows, int k,
                          int64_t batch, float* out, rs_stream_t stream);
int rs_ffm_fwd(const void* ids, int id_kind, int64_t id_stride,
               const float* dense, int64_t dense_stride, int nd,
               const float* v, const float* w, const float* w0,
               const int64_t* field_offsets, const int64_t* field_vocab,
               int n_fields, int k, int n_sigmoid, float* out, int64_t batch,
               int* err_flag, rs_stream_t stream);

/* ------------------------------------------ training (§8(f) rank 4)
 * rs_fm_train_step: one SGD step of the FM model (model/fm.py:14-23 +
 * utils/compile_fit.py:9-15) on a batch in compact form — dense [B, nd] and
 * label codes ids [B, F] standing for x = [dense | one-hot] (one-hot column
 * nd + field_offsets[c] + id, utils/dataset.py:47-48) — with the FMLayer
 * weights w0 (1), w1 (n_rows), v (n_rows, k) updated in place:
 *   y = w0 + x@w1 + 0.5 sum_f [(x@v)_f^2 - (x^2@v^2)_f],
 *   dL/dy_b = (sigmoid(y_b) - labels_b) / B   (Keras binary_crossentropy on
 *   the sigmoid's logits, batch mean), l2 regularisers l2_w on w1 and l2_v
 *   on v (FMLayer.build, layer/interaction.py:97-104), SGD with rate lr.
 * Every row decays (the regulariser's dense gradient); the looked-up rows
 * get their summed gradient through a deterministic sort + segmented sum.
 * loss (optional, [B]): per-sample cross-entropy before the step.
 * workspace: rs_fm_train_workspace_size(B, F, k, nd) bytes (device).       */
int64_t rs_fm_train_workspace_size(int64_t batch, int n_fields, int k, int nd);
int rs_fm_train_step(const void* ids, int id_kind, int64_t id_stride,
                     const float* dense, int64_t dense_stride, int nd,
                     const int64_t* field_offsets, const int64_t* field_vocab,
                     int n_fields, int k, float* w0, float* w1, float* v,
                     int64_t n_rows, const float* labels, int64_t batch,
                     float lr, float l2_w, float l2_v, void* workspace,
                     float* loss, int* err_flag, rs_stream_t stream);

/* rs_dropout: DNNLayer's Dropout(rate) in training (layer/interaction.py:35,44;
 * active under compile_fit's model.fit, utils/compile_fit.py:14), in place on
 * x[rows, cols] (row stride ld): x <- keep ? x / (1 - rate) : 0 with
 * keep = u >= rate, u from Philox4x32-10 (key = seed, counter =
 * (offset + row*cols + col) / 4, word (offset + e) % 4, u = (word >> 8) 2^-24).
 * offset % 4 == 0; callers advance it by 4*ceil(rows*cols/4) per draw.  The
 * same (seed, offset) applied to dL/dx is the backward (the mask is never
 * stored).  TF's own draws cannot be reproduced; oracle.dropout_multiplier
 * restates this generator exactly.                                          */
int rs_dropout(float* x, int64_t ld, int64_t rows, int64_t cols, float rate,
               uint64_t seed, uint64_t offset, rs_stream_t stream);
/* rs_dropout_at: the same draw at offset *base + offset, with the base read
 * on the device (a per-generator counter in device memory), so a captured
 * hipGraph replays fresh masks; rs_dropout_advance adds inc (a multiple of 4)
 * to *base on the stream — the training steps call it once, after the
 * backward's redraws, with the step's total.                                */
int rs_dropout_at(float* x, int64_t ld, int64_t rows, int64_t cols, float rate,
                  uint64_t seed, const uint64_t* base, uint64_t offset,
                  rs_stream_t stream);
int rs_dropout_advance(uint64_t* base, uint64_t inc, rs_stream_t stream);

/* DeepFM training (model/deepFM.py + utils/compile_fit.py; the host layer
 * DeepFM.train_step composes these with rs_embed_gather / rs_dense_fwd /
 * rs_fm_fwd):
 * rs_gemm: C[M,N] = alpha op(A)[M,K] op(B)[K,N] + beta C (row-major; op =
 *  transpose when trans_*), then C *= (mask > 0) if mask (ReLU backward);
 *  deterministic (each output's K sum in one fixed order).  With a
 *  workspace of rs_gemm_workspace_size(M, N, K) bytes (0 = not needed) a
 *  launch of few output tiles splits K into slices summed in slice order.
 * rs_col_sum: out[n] = sum_m A[m,n] (bias gradients), fixed-order trees.
 * rs_sgd_update: w -= lr (grad + 2 l2 w) (Keras SGD + l2 regulariser).
 * rs_head_grad: z = c_fm fm + c_dnn dnn (DeepFM: 0.5, 0.5),
 *  g = (sigmoid(z) - t)/B -> g_fm = c_fm g, g_dnn = c_dnn g, loss (optional).
 * rs_fm_x_grad: dx[b,i] += g_b (w1_i + sum_f v_if s_bf - x_bi sum_f v_if^2)
 *  (FMLayer w.r.t. its input; s = x @ v).
 * rs_fm_param_grads: dw1 = x^T g, dv = x^T (g s) - (x^2)^T g * v, dw0 =
 *  sum g (no l2 terms; kfm <= 32).
 * rs_embedding_sgd: table[off_c + id(b,c)] -= lr * grad[b, c*k : c*k+k]
 *  summed over duplicate rows in lookup order (stable sort + segmented sum:
 *  Keras' IndexedSlices scatter-add); workspace:
 *  rs_embedding_sgd_workspace_size(batch * n_fields) bytes.                 */
/* rs_sort_pairs_u32: stable ascending sort of (key, val) pairs by the low
 *  `bits` bits of key (LSD radix, 8 bits a pass; equal keys keep their input
 *  order), the grouping step of every row-sparse scatter-add here
 *  (rs_embedding_sgd, rs_fm_train_step, rs_shard_dedup_route beyond 4096
 *  samples) — Keras' IndexedSlices accumulation groups the same rows
 *  (utils/compile_fit.py:9-15 via SGD on the Embedding); in != out,
 *  workspace: rs_sort_pairs_workspace_size(n) bytes.
 * rs_inclusive_sum_i32: out[i] = in[0] + ... + in[i] (in == out allowed),
 *  workspace: rs_inclusive_sum_workspace_size(n) bytes.                    */
int64_t rs_sort_pairs_workspace_size(int64_t n);
int rs_sort_pairs_u32(const uint32_t* key_in, const uint32_t* val_in,
                      uint32_t* key_out, uint32_t* val_out, int64_t n,
                      int bits, void* workspace, rs_stream_t stream);
int64_t rs_inclusive_sum_workspace_size(int64_t n);
int rs_inclusive_sum_i32(const int32_t* in, int32_t* out, int64_t n,
                         void* workspace, rs_stream_t stream);
int64_t rs_gemm_workspace_size(int64_t M, int64_t N, int64_t K);
int rs_gemm(int trans_a, int trans_b, int64_t M, int64_t N, int64_t K,
            float alpha, const float* A, int64_t lda, const float* B,
            int64_t ldb, float beta, float* C, int64_t ldc, const float* mask,
            int64_t ldm, void* workspace, int64_t workspace_bytes,
            rs_stream_t stream);
int rs_col_sum(const float* A, int64_t lda, int64_t M, int64_t N, float* out,
               rs_stream_t stream);
/* rs_col_sum over many rows: slices of 256 rows (fewer, down to 16, when
 * that leaves < 64 slices) summed into a workspace of
 * rs_col_sum_workspace_size(M, N) bytes, then the slices in order
 * (deterministic); without room (or one slice) it is rs_col_sum.           */
int64_t rs_col_sum_workspace_size(int64_t M, int64_t N);
int rs_col_sum_split(const float* A, int64_t lda, int64_t M, int64_t N,
                     float* out, void* workspace, int64_t workspace_bytes,
                     rs_stream_t stream);
int rs_sgd_update(float* w, const float* grad, int64_t n, float lr, float l2,
                  rs_stream_t stream);
/* rs_sgd_update over `count` tensors (host arrays of device pointers, sizes
 * and per-tensor l2) in one launch per 32 tensors: the optimizer step of a
 * model's dense parameters (Keras' SGD.apply_gradients over the variable
 * list, utils/compile_fit.py:11 / model/pnn.py:81), same arithmetic.       */
int rs_sgd_update_multi(int count, float* const* w, const float* const* grad,
                        const int64_t* n, const float* l2, float lr,
                        rs_stream_t stream);
int rs_head_grad(const float* fm, const float* dnn, const float* labels,
                 int64_t batch, float c_fm, float c_dnn, float* g_fm,
                 float* g_dnn, float* loss, rs_stream_t stream);
/* PNN training (the reference's GradientTape loop, model/pnn.py:74-85):
 * rs_bce_prob_grad: tf.reduce_mean(losses.binary_crossentropy(y[B],
 *  pre[B,1])) on the DNN LOGIT as Keras computes it — pre clipped to
 *  [1e-7, 1-1e-7], labels broadcast against the [B,1] output (per sample i
 *  the mean over j of BCE(y_j, pre_i)): loss[i] = -(ybar log(q_i+eps) +
 *  (1-ybar) log(1-q_i+eps)), g[i] = dL/dpre_i (0 outside the clip range).
 * rs_inner_product_bwd: InnerProductLayer backward (layer/interaction.py:
 *  170-183): demb[b,i,:] = dflat[b,i,:] + sum_{j!=i} dinner[b,p(i,j)]
 *  emb[b,j,:] (p = the row-major pair index); 2 <= n_fields <= 64, k <= 64. */
int rs_bce_prob_grad(const float* pred, int64_t pred_stride,
                     const float* labels, int64_t batch, float* g, float* loss,
                     rs_stream_t stream);
int rs_inner_product_bwd(const float* emb, int64_t emb_stride,
                         const float* dinner, int64_t dinner_stride,
                         const float* dflat, int64_t dflat_stride, int n_fields,
                         int k, int64_t batch, float* demb, int64_t demb_stride,
                         rs_stream_t stream);
/* NFM Bi-Interaction backward (model/nfm.py:28, 3-D embeddings; NFM
 * training): demb[b, f*k + c] = dbi[b, c] (S_bc - e_bfc), S = sum_f e_f.      */
int rs_bi_interaction_bwd(const float* emb, int64_t emb_stride,
                          const float* dbi, int64_t dbi_stride, int n_fields,
                          int k, int64_t batch, float* demb,
                          int64_t demb_stride, rs_stream_t stream);
/* OuterProductLayer backward (layer/interaction.py:200-215, PNN modes
 * 'outer' / 'both'): o_p = e_j^T W_p e_i, W_p[a][c] = W[a,p,c], W [k, P, k].
 * rs_outer_product_bwd ADDS to demb[b, f*k ..]: sum_{j>f} g_p e_j W_p +
 *  sum_{i<f} g_p e_i W_p^T (g = dout[b, p], pairs in order).
 * rs_outer_product_w_grad: dW[a,p,c] = sum_b g_bp e_j[b,a] e_i[b,c].
 * 2 <= n_fields <= 64, 1 <= k <= 16; fp32 MFMA, deterministic.              */
int rs_outer_product_bwd(const float* emb, int64_t emb_stride,
                         const float* dout, int64_t dout_stride, const float* W,
                         int n_fields, int k, int64_t batch, float* demb,
                         int64_t demb_stride, rs_stream_t stream);
int rs_outer_product_w_grad(const float* emb, int64_t emb_stride,
                            const float* dout, int64_t dout_stride,
                            int n_fields, int k, int64_t batch, float* dW,
                            rs_stream_t stream);
/* The product layers' backward past 64 fields (PNN with FGCNN: the layers see
 * z = [embed | new fields], 83 fields at the defaults) — the counterpart of
 * rs_product_fwd.  z [B, F, k] rows z_stride floats apart; dx = the DNN's
 * input gradient, one row [dflat (F*k) | dinner (P, if inner) | douter (P, if
 * outer)] per sample, dx_stride floats apart; W = the RAW [k, P, k] tensor
 * (not the rs_outer_prepare image).  2 <= n_fields <= 128, 1 <= k <= 16.
 * rs_product_bwd (outer iff W != NULL; inner = 0 and W = NULL is refused):
 *  ONE launch WRITES dz[b,i,:] = dflat + sum_{j!=i} dinner_p(i,j) z_j +
 *  sum_{j>i} g_p z_j W_p + sum_{j<i} g_p z_j W_p^T; one fp32 MFMA chain per
 *  (sample tile, field) over the other fields in order, 16 samples per
 *  workgroup, 8 or 4 where 16 rows of z pass 64 KB of LDS; no atomics.
 * rs_product_w_grad (always outer; `inner` only places the douter columns):
 *  dW[a,p,c] = sum_b g_bp z_j[b,a] z_i[b,c], one workgroup per pair.
 * A refusal launches nothing; batch 0 returns RS_OK.                        */
int rs_product_bwd(const float* z, int64_t z_stride, const float* dx,
                   int64_t dx_stride, int n_fields, int k, int inner,
                   const float* W, int64_t batch, float* dz, int64_t dz_stride,
                   rs_stream_t stream);
int rs_product_w_grad(const float* z, int64_t z_stride, const float* dx,
                      int64_t dx_stride, int n_fields, int k, int inner,
                      int64_t batch, float* dW, rs_stream_t stream);
/* FGCNN conv stack backward (the layers of rs_fgcnn_conv_fwd, same
 * configuration arguments), ONE launch for the stack plus a fixed-order finish
 * of the weight gradients.  Saved from the forward: z[b, 0:F*k] (the rows) and
 * ws (every layer's pooled map).  dws [B, ws_size] = dL/d(pooled maps) from
 * the recombination Dense layers.  Per sample and layer, top down, in LDS: the
 * pooled gradient (dws_i + the input gradient of the layer above) goes to the
 * FIRST pool member attaining the maximum (members recomputed in fp32), times
 * 1 - p^2 (p the saved pooled value); rows the pool dropped get zero.  Then
 * db = sum dY, dW[t,c,n] = sum Xpad[h+t,d,c] dY[h,d,n], and dX = the
 * transposed convolution.  dX_0 is ADDED into de[b, 0:F*k] (rows de_stride
 * apart).  dconv_w[i] / dconv_b[i] (host arrays of device pointers, the
 * parameters' shapes) are WRITTEN: per-workgroup partial rows in `workspace`
 * (rs_fgcnn_conv_bwd_workspace_size bytes for this batch), summed in row
 * order; no atomics, bitwise reproducible.
 * rs_fgcnn_conv_bwd_workspace_size returns -1 (error string set) for a
 * configuration rs_fgcnn_workspace_size refuses or whose backward tile — one
 * layer's kernel, padded input map, padded dY map and the carried gradient —
 * passes 128 KB of LDS (the defaults fit at k = 8, 16 and 32).              */
int64_t rs_fgcnn_conv_bwd_workspace_size(int n_fields, int k, int n_layers,
                                         const int* filters,
                                         const int* kernel_width,
                                         const int* pooling_width,
                                         int64_t batch);
int rs_fgcnn_conv_bwd(const float* z, int64_t z_stride, const float* ws,
                      int64_t ws_stride, const float* dws, int64_t dws_stride,
                      int n_fields, int k, int n_layers, const int* filters,
                      const int* kernel_width, const int* pooling_width,
                      const float* const* conv_w, float* de, int64_t de_stride,
                      float* const* dconv_w, float* const* dconv_b,
                      void* workspace, int64_t workspace_bytes, int64_t batch,
                      rs_stream_t stream);
/* DIN training (compile_fit on model/din.py:56-95, training=True; the host
 * layer DIN.train_step composes these with rs_dense_fwd / rs_gemm /
 * rs_col_sum / rs_sgd_update / rs_embedding_sgd):
 * rs_din_att_concat: out[b*T+t] = [q_b, s_bt, q_b - s_bt, q_b * s_bt]
 *  (the attention unit input, layer/interaction.py:381-391); item [B,K],
 *  seq [B*T,K], out [B*T,4K] dense rows.
 * rs_din_att_concat_bwd: from d = dL/dout: dq[b] += sum_t (d0 + d2 + s d3)
 *  (row stride dq_stride), dseq[b*T+t] += d1 - d2 + q d3.
 * rs_prelu_rows_fwd / _bwd: Keras PReLU on rows, y = max(z,0) +
 *  alpha[(r mod period), c] min(z,0) (the attention's [T,h] alphas: period
 *  T; a Dense layer's [N]: period 1); bwd writes dz = dy (z>0 ? 1 : alpha)
 *  and dalpha[p,c] = sum_{r = p mod period} dy min(z,0) (the split column
 *  sums below; M a multiple of period); workspace:
 *  rs_prelu_rows_bwd_workspace_size(M, N, period) bytes.
 * rs_masked_softmax_pool: s = score, or -2^32+1 where hist[b,0..T) == 0
 *  (the first behaviour feature, model/din.py:80); a = softmax_T(s) [B,T];
 *  out[b] = sum_t a_t seq[b*T+t] (:396-404).  T <= 512.
 * rs_masked_softmax_pool_bwd: from datt: ds[b,t] = live ? a_t (da_t -
 *  sum_s a_s da_s) : 0 with da_t = datt . seq_t; dseq[b*T+t] = a_t datt
 *  (stored, not accumulated).
 * rs_bn_train_fwd: BatchNormalization in training mode — per column the
 *  batch mean and biased variance into mean / var, y = (x - mean)
 *  rsqrt(var + eps) gamma + beta, and (when non-NULL) moving = momentum
 *  moving + (1 - momentum) batch stat.
 * rs_bn_train_bwd: dgamma = sum dy xhat, dbeta = sum dy, dx = gamma
 *  rsqrt(var+eps) (dy - dbeta/B - xhat dgamma/B).                          */
int rs_din_att_concat(const float* item, const float* seq, int64_t batch,
                      int T, int K, float* out, rs_stream_t stream);
int rs_din_att_concat_bwd(const float* d, const float* item, const float* seq,
                          int64_t batch, int T, int K, float* dq,
                          int64_t dq_stride, float* dseq, rs_stream_t stream);
int rs_prelu_rows_fwd(const float* z, int64_t M, int N, const float* alpha,
                      int period, float* y, rs_stream_t stream);
int64_t rs_prelu_rows_bwd_workspace_size(int64_t M, int N, int period);
int rs_prelu_rows_bwd(const float* z, const float* dy, int64_t M, int N,
                      const float* alpha, int period, float* dz,
                      float* dalpha, void* workspace, int64_t workspace_bytes,
                      rs_stream_t stream);
/* rs_din_att_prelu_bwd: the whole backward of the PReLU attention unit
 * with two hidden layers (layer/interaction.py:366-395; default (80, 40)) in
 * one launch + a fixed-order partial sum: from h0 [B*T, K0] (the concat
 * [q, k, q-k, q*k]), the pre-activations z1 [B*T, h1], z2 [B*T, h2], ds
 * [B*T] (dL/dscore), the kernels W1 [K0, h1], W2 [h1, h2], the PReLU alphas
 * [T, h1] / [T, h2] and the score kernel wo [h2], writes dh0 [B*T, K0] and
 * dW1, db1, dalpha1, dW2, db2, dalpha2, dwo [h2], dbo [1].  Shapes with T,
 * K0, h1, h2 <= 128, multiples of 4, whose sample fits in LDS:
 * rs_din_att_prelu_bwd_workspace_size returns -1 for the others.           */
/* rs_din_att_prelu_fwd: the unit's forward under fit for the same shapes:
 * z1 = h0 W1 + b1, z2 = prelu(z1; alpha1) W2 + b2 (kept for the backward),
 * score = prelu(z2; alpha2) wo + bo [B*T], one launch.                      */
int rs_din_att_prelu_fwd(const float* h0, const float* W1, const float* b1,
                         const float* alpha1, const float* W2,
                         const float* b2, const float* alpha2,
                         const float* wo, const float* bo, int64_t batch,
                         int T, int K0, int h1, int h2, float* z1, float* z2,
                         float* score, rs_stream_t stream);
int64_t rs_din_att_prelu_bwd_workspace_size(int64_t batch, int T, int K0,
                                            int h1, int h2);
int rs_din_att_prelu_bwd(const float* h0, const float* z1, const float* z2,
                         const float* ds, const float* W1, const float* W2,
                         const float* alpha1, const float* alpha2,
                         const float* wo, int64_t batch, int T, int K0, int h1,
                         int h2, float* dh0, float* dW1, float* db1,
                         float* dalpha1, float* dW2, float* db2,
                         float* dalpha2, float* dwo, float* dbo,
                         void* workspace, int64_t workspace_bytes,
                         rs_stream_t stream);
int rs_masked_softmax_pool(const float* score, const void* hist,
                           int hist_kind, int64_t hist_stride,
                           const float* seq, int64_t batch, int T, int K,
                           float* a, float* out, int64_t out_stride,
                           rs_stream_t stream);
int rs_masked_softmax_pool_bwd(const float* a, const void* hist,
                               int hist_kind, int64_t hist_stride,
                               const float* seq, const float* datt,
                               int64_t datt_stride, int64_t batch, int T,
                               int K, float* ds, float* dseq,
                               rs_stream_t stream);
int rs_bn_train_fwd(const float* x, int64_t x_stride, int64_t batch, int D,
                    const float* gamma, const float* beta, float eps,
                    float momentum, float* moving_mean, float* moving_var,
                    float* mean, float* var, float* y, int64_t y_stride,
                    rs_stream_t stream);
int rs_bn_train_bwd(const float* x, int64_t x_stride, int64_t batch, int D,
                    const float* mean, const float* var, const float* gamma,
                    float eps, const float* dy, int64_t dy_stride, float* dx,
                    int64_t dx_stride, float* dgamma, float* dbeta,
                    rs_stream_t stream);
/* Dice in training (layer/interaction.py:416-425 under fit, DIN with
 * att_attention / dnn_activation 'dice'), x [M, N] dense rows (the
 * attention's [B, T, 4k] as [B*T, 4k]): its BatchNormalization(center=False,
 * scale=False) with the batch's per-column mean and biased variance (into
 * mean / var, moving averages moved with momentum when non-NULL);
 * y = alpha (1 - p) x + p x, p = sigmoid((x - mean) rsqrt(var + eps)).
 * rs_dice_train_bwd: dx = dy (alpha (1-p) + p) + the batch-norm backward of
 * dL/dxhat = dy (1 - alpha) x p (1 - p); dalpha = sum dy (1 - p) x.
 * Workspace: rs_dice_train_workspace_size(M, N) bytes.  Deterministic.     */
int64_t rs_dice_train_workspace_size(int64_t M, int N);
int rs_dice_train_fwd(const float* x, int64_t M, int N, const float* alpha,
                      float eps, float momentum, float* moving_mean,
                      float* moving_var, float* mean, float* var, float* y,
                      void* workspace, int64_t workspace_bytes,
                      rs_stream_t stream);
int rs_dice_train_bwd(const float* x, int64_t M, int N, const float* alpha,
                      const float* mean, const float* var, float eps,
                      const float* dy, float* dx, float* dalpha,
                      void* workspace, int64_t workspace_bytes,
                      rs_stream_t stream);
/* rs_head_grad with g = scale (sigmoid(z) - t) (scale > 0): the sharded
 * DeepFM step's local batch is a 1/world share of the global batch mean,
 * scale = 1 / (world * batch).                                             */
int rs_head_grad_scaled(const float* fm, const float* dnn, const float* labels,
                        int64_t batch, float c_fm, float c_dnn, float scale,
                        float* g_fm, float* g_dnn, float* loss,
                        rs_stream_t stream);
int rs_fm_x_grad(const float* x, int64_t ldx, const float* s, const float* w1,
                 const float* v, int64_t batch, int d, int kfm, const float* g,
                 float* dx, int64_t lddx, rs_stream_t stream);
int rs_fm_param_grads(const float* x, int64_t ldx, const float* s,
                      const float* v, int64_t batch, int d, int kfm,
                      const float* g, float* dw1, float* dv, float* dw0,
                      rs_stream_t stream);
/* rs_fm_param_grads with s rows lds floats apart and g ldg floats apart
 * (the sharded backward's interleaved [s | g] records); dw0 NULL = skip.   */
int rs_fm_param_grads_strided(const float* x, int64_t ldx, const float* s,
                              int64_t lds, const float* g, int64_t ldg,
                              const float* v, int64_t batch, int d, int kfm,
                              float* dw1, float* dv, float* dw0,
                              rs_stream_t stream);
/* CrossNet training (layer/interaction.py:75-83, DCN.train_step):
 * rs_cross_train_fwd: x_{l+1} = x0 (x_l . w_l) + b_l + x_l for l < L;
 *  W, b [L, d] (row l = w_l, b_l); keeps xs [L, B, d] (x_1 .. x_L) and
 *  g [L, B] (g_l = x_l . w_l); x_L also to xl_out (row stride ldo; may be
 *  NULL).  d <= 2048.
 * rs_cross_train_bwd: from dxl = dL/dx_L: deltas [L, B, d] (delta_{l+1} for
 *  db_l = sum_b delta_{l+1}), s [L, B] (s_l = x0 . delta_{l+1}, for dw_l =
 *  sum_b s_l x_l), and dx += delta_0 + sum_l g_l delta_{l+1} (dL/dx0).      */
int rs_cross_train_fwd(const float* x0, int64_t ldx, int d, int n_layers,
                       const float* W, const float* b, int64_t batch,
                       float* xs, float* g, float* xl_out, int64_t ldo,
                       rs_stream_t stream);
int rs_cross_train_bwd(const float* x0, int64_t ldx, int d, int n_layers,
                       const float* W, int64_t batch, const float* g,
                       const float* dxl, int64_t lddxl, float* deltas,
                       float* s, float* dx, int64_t lddx,
                       rs_stream_t stream);
/* rs_embedding_sgd with the gradient row of lookup (b, c) at grad[b *
 * grad_stride + c * grad_field_stride] (k for one row per lookup; 0 for one
 * row per sample shared by all its fields — the FFM step).                 */
int rs_embedding_sgd_strided(float* table, int64_t n_rows, int k,
                             const void* ids, int id_kind, int64_t id_stride,
                             const int64_t* field_offsets,
                             const int64_t* field_vocab, int n_fields,
                             int64_t batch, const float* grad,
                             int64_t grad_stride, int64_t grad_field_stride,
                             float lr, void* workspace, int* err_flag,
                             rs_stream_t stream);
/* FFM training (compile_fit on FFM, model/ffm.py:20-22; FFM.train_step
 * composes it with rs_gemm / rs_col_sum / rs_sgd_update / rs_l2_decay /
 * rs_embedding_sgd_strided): rs_ffm_train_fwd computes, per sample, Fm[f,c]
 * = sum_i x_i v[i,f,c] (v [feature_num, nd+F, k]; the nd dense rows and row
 * nd + field_offsets[c] + id of each field, an out-of-range id being
 * tf.one_hot's zero row), z = w0 + x.w + 0.5(|sum_f Fm_f|^2 - sum_f |Fm_f|^2),
 * g[b] = (sigmoid(z) - t)/B, loss[b] (optional) and G[b, f*k + c] =
 * g (T_c - Fm[f,c]), T = sum_f Fm_f.  (nd + F) * k <= 4096, k <= 64.
 * rs_l2_decay: w -= lr * 2 l2 w over n floats (Keras l2 on every row).      */
int rs_ffm_train_fwd(const void* ids, int id_kind, int64_t id_stride,
                     const float* dense, int64_t dense_stride, int nd,
                     const float* v, const float* w, const float* w0,
                     const int64_t* field_offsets, const int64_t* field_vocab,
                     int n_fields, int k, const float* labels, int64_t batch,
                     float* G, float* g, float* loss, rs_stream_t stream);
int rs_l2_decay(float* w, int64_t n, float lr, float l2, rs_stream_t stream);
int64_t rs_embedding_sgd_workspace_size(int64_t n_lookups);
int rs_embedding_sgd(float* table, int64_t n_rows, int k, const void* ids,
                     int id_kind, int64_t id_stride,
                     const int64_t* field_offsets, const int64_t* field_vocab,
                     int n_fields, int64_t batch, const float* grad,
                     int64_t grad_stride, float lr, void* workspace,
                     int* err_flag, rs_stream_t stream);
/* AFM training (compile_fit on AFM, utils/compile_fit.py:9-15 on
 * model/afm.py:15-18; AFM.train_step composes it with rs_gemm / rs_col_sum /
 * rs_sgd_update_multi / rs_embedding_sgd): rs_afm_train_fwd is
 * rs_embed_pair_pool_fwd's forward (same ids / table / mode arguments: mode 0
 * sum = 'att', 1 mean = 'avg', 2 max, n_fields <= 32 for max; 1 <= k <= 64)
 * AND the backward down to the rows, in one launch with the rows in
 * registers.  With x = the pooled pair products, z = x.head_w + head_b[0],
 * s = sigmoid(z) and u = the input of the last of the n_sigmoid (1 or 2)
 * sigmoids (u = z, or u = s: Keras takes it as the BCE logit):
 *   pooled[b*pooled_stride + c] = x_c;  prob[b] = sigmoid(u) (optional);
 *   loss[b] = max(u,0) - u t + log1p(exp(-|u|)) (optional), t = labels[b];
 *   g[b] = dL/dz = (sigmoid(u) - t)/batch, times s(1-s) with two sigmoids;
 *   drows[b*drows_stride + f*k + c] = dL/d(row of field f)_c, the layout
 *   rs_embedding_sgd reads: g w_c (S_c - e_fc) with S = sum_f e_f (sum), the
 *   same / P (mean), or for max g w_c e_{j*}c at i*, g w_c e_{i*}c at j* and 0
 *   elsewhere, (i*, j*) the arg-max pair of (b, c) — a tie goes to the first
 *   pair in row-major order (TF splits it evenly among the tied pairs).
 * Every element of drows[b, 0 : n_fields*k] is written (no pre-zeroing); one
 * field has no pair (x = 0, drows = 0, g still produced).  An out-of-range id
 * is the forward's zero row: it sets RS_FLAG_BAD_ID and its own block of
 * drows is 0.  dL/dhead_w = pooled^T g and dL/dhead_b = sum_b g are left to
 * rs_gemm / rs_col_sum.  No atomics: run-to-run bit-identical.              */
int rs_afm_train_fwd(const void* ids, int id_kind, int64_t id_stride,
                     const float* table, const int64_t* field_offsets,
                     const int64_t* field_vocab, int n_fields, int k, int mode,
                     const float* head_w, const float* head_b, int n_sigmoid,
                     const float* labels, int64_t batch, float* pooled,
                     int64_t pooled_stride, float* prob, float* g, float* loss,
                     float* drows, int64_t drows_stride, int* err_flag,
                     rs_stream_t stream);

/* -------------------------------------- row-sharded lookup (§8(e), cfg 5)
 * Global row of (b,c) = field_offsets[c] + id(b,c).  Rows are split across
 * `world` ranks in blocks of `rows_per_rank` (owner = row / rows_per_rank).
 *  rs_shard_bucketize: counts[r] = #lookups owned by rank r; perm[i] = the
 *   position of lookup i (= b*F + c) in owner-major order; send_rows[perm[i]]
 *   = local row index on the owner.  Stable within each owner.  An id outside
 *   [0, vocab) sets *err_flag and is kept as a lookup of owner 0 with local
 *   row -1 (counted in counts[0], perm still a permutation of 0 .. n-1, its
 *   send_rows word -1: rs_gather_rows serves it as a zero row), so the packed
 *   exchange keeps one word and one row per lookup.
 *   workspace: rs_shard_workspace_size(batch*n_fields, world) bytes, device,
 *   zero-filled once when allocated (its tail holds the control words of the
 *   one-pass slotted kernel, which leaves them ready for the next call); one
 *   workspace per stream — concurrent calls must not share it.
 *  rs_gather_rows: out[i] = table[rows[i]] (k floats), local shard.
 *  rs_unpermute_rows: dst[i] = src[perm[i]] (k floats per row).            */
int64_t rs_shard_workspace_size(int64_t n_lookups, int world);
int rs_shard_bucketize(const void* ids, int id_kind, int64_t id_stride,
                       const int64_t* field_offsets, const int64_t* field_vocab,
                       int n_fields, int64_t batch, int64_t rows_per_rank,
                       int world, int32_t* counts, int32_t* perm,
                       int32_t* send_rows, void* workspace, int* err_flag,
                       rs_stream_t stream);

/* Fixed-capacity ("slotted") variant for a host-sync-free exchange: every
 * (rank -> owner) message is exactly `cap` slots, so both all-to-alls have
 * equal, host-known splits.  send_slots [world*cap]: slots not used by this
 * step keep their previous content (fill the buffer with -1 once, when it is
 * allocated: -1 is served as a zero row, a stale slot as a valid row of the
 * owner's shard that no lookup reads); slot_of [B*F]: the slot of lookup
 * b*F+c, or -1 when its owner's slots overflowed (*overflow_flag set; redo the
 * step with the exact protocol) or its id is out of range (*err_flag set).
 * An out-of-range id is no lookup of any owner: it takes no slot, writes no
 * send word, is not counted in counts[] (counts[o] = the valid lookups of
 * owner o, overflowed ones included) and cannot push a valid lookup past
 * `cap`.
 * The returned rows are then addressed by slot_of as int32 ids of a single
 * [world*cap, k] table: rs_embed_fm_fwd(ids = slot_of, offsets 0, vocab
 * world*cap) computes the FM straight from the exchange buffer.
 * One launch: stable per-owner ranks in LDS + a decoupled look-back over the
 * preceding blocks' per-owner totals (single-pass chained scan).            */
int rs_shard_slot_bucketize(const void* ids, int id_kind, int64_t id_stride,
                            const int64_t* field_offsets,
                            const int64_t* field_vocab, int n_fields,
                            int64_t batch, int64_t rows_per_rank, int world,
                            int cap, int32_t* counts, int32_t* slot_of,
                            int32_t* send_slots, void* workspace, int* err_flag,
                            int* overflow_flag, rs_stream_t stream);
int rs_gather_rows(const float* table, int64_t n_rows, int k,
                   const int32_t* rows, int64_t n, float* out, int* err_flag,
                   rs_stream_t stream);
int rs_unpermute_rows(const float* src, const int32_t* perm, int k, int64_t n,
                      float* dst, rs_stream_t stream);

/* ------------------- row-sharded FM, partial protocol (§8(e), default)
 * A block split of the concatenated table gives every owner o a contiguous
 * FIELD range [field_lo(o), field_lo(o) + n_owned(o)).  Instead of returning
 * 64-B rows, the owner returns per-sample FM partials over the fields it
 * holds (the FM's first stage x@[v|w1] and x^2@|v|^2 is linear in the rows),
 * and the requester finishes the FM (FMLayer.call, layer/interaction.py:
 * 106-114; EmbedLayer.call, layer/core.py:273-280, for the lookup):
 *  rs_fm_partial_width(kfm): floats per partial record, P = roundup(kfm+2, 4):
 *   [s_0 .. s_{kfm-1}, x@w1, sum_i x_i^2 |v_i|^2, 0-pad].
 *  rs_shard_field_route: owner_fields [world][2] int32 = (field_lo, n_owned)
 *   per owner; send = world*batch records of rec_stride int32 words (owner-
 *   major), word j < slot_stride (slot_stride >= every n_owned) of record
 *   (o, b) = local row of lookup (b, field_lo(o)+j) when o owns it, else -1.
 *   Those words are all written; words >= slot_stride are left untouched;
 *   out-of-range id -> *err_flag.
 *  rs_shard_owner_fm: local_rows = n_pairs records of rec_stride words (the
 *   received messages, requester-major), the owner's shard [shard_rows, k]
 *   and the packed FM image of the WHOLE model (rs_fm_prepare with nd,
 *   n_fields) -> partial records (P floats, partial_stride floats apart) over
 *   fields field_lo .. field_lo+n_owned-1 (-1 rows contribute 0; a local row
 *   >= shard_rows sets *err_flag).
 *  rs_shard_fm_combine: partial records [world][batch] (partial_stride floats
 *   apart, one block per owner) + dense [batch, nd] -> logit[batch]; owners
 *   summed in rank order.
 *  A pipelined exchange interleaves both messages in ONE buffer: record
 *   (peer, b) = [slot_stride row ids of batch t | P partial floats of batch
 *   t-1], rec_stride = partial_stride = slot_stride + P, partials at +slot_stride
 *   words: one all-to-all per batch (sharded.py forward_stream).            */
int rs_fm_partial_width(int kfm);
int rs_shard_field_route(const void* ids, int id_kind, int64_t id_stride,
                         const int64_t* field_offsets,
                         const int64_t* field_vocab, int n_fields,
                         int64_t batch, int64_t rows_per_rank, int world,
                         const int32_t* owner_fields, int slot_stride,
                         int64_t rec_stride, int32_t* send, int* err_flag,
                         rs_stream_t stream);
/* Row protocol on the same field-range records (ShardedDeepFM, config 5: the
 * DNN needs every row at the requester, so rows come back instead of FM
 * partials; EmbedLayer.call, layer/core.py:273-280, sharded):
 *  rs_shard_row_route: rs_shard_field_route with rec_stride = slot_stride,
 *   plus slot_of[b*n_fields + c] = the record word (o*batch + b)*slot_stride
 *   + j of lookup (b, c) (o = its owner, j = c - field_lo(o)), or -1 for an
 *   out-of-range id (*err_flag set).  The owner answers the received words
 *   with rs_gather_rows (-1 -> zero row) into [world*batch*slot_stride, k];
 *   after the row all-to-all, lookup (b, c)'s row is got[slot_of[b*F + c]],
 *   so rs_deepfm_fwd(ids = slot_of, offsets 0, vocab world*batch*slot_stride,
 *   table = got) runs the whole DeepFM forward straight from the exchange
 *   buffer.  Fixed sizes, no scan, no capacity, no overflow.                 */
/* Row-id deduplication before the sharded row exchange (ShardedDeepFM with
 * dedup): the rank sends each owner only the DISTINCT rows it needs, in a
 * fixed-capacity message of `cap` words per owner (send[world*cap]: distinct
 * local row u of owner o at word o*cap + u, in row order; unused words -1,
 * served as zero rows by rs_gather_rows).  slot_of[b*n_fields + c] = o*cap +
 * u, the reply row of lookup (b, c) after the row all-to-all (rs_deepfm_fwd
 * with ids = slot_of, vocab world*cap, reads the exchange buffer unchanged);
 * -1 for a bad id (*err_flag) or a distinct row past `cap` (*overflow_flag:
 * the caller redoes the step without dedup).  For
 * batch <= 4096, n_fields <= 1024 and world <= 4096, one workgroup per
 * field dedups its lookups in an LDS hash table and numbers each owner's
 * distinct rows field by field in order of first occurrence (the
 * concatenated table's fields occupy increasing, disjoint row ranges;
 * field_offsets[c] + field_vocab[c] > field_offsets[c+1] sets
 * RS_FLAG_LAYOUT), and a second launch scatters — no sort; larger batches
 * use a device-wide radix sort and number the rows in row order.  Either
 * way the numbering is deterministic.
 * rs_shard_dedup_grad (backward, same workspace, after the route of the same
 * step): dst[slot] = sum of the gradient rows grad[b*grad_stride + c*k ..]
 * of every lookup of that distinct row, in lookup order (the lookups grouped
 * by row first — on the hash path by a per-field launch of its own — then
 * summed in fixed chunk pieces, so hot rows stay parallel) — one gradient
 * row per distinct row travels back to its owner.  Workspace: rs_shard_dedup_workspace_size(batch*n_fields,
 * world) bytes.                                                            */
int64_t rs_shard_dedup_workspace_size(int64_t n_lookups, int world);
int rs_shard_dedup_route(const void* ids, int id_kind, int64_t id_stride,
                         const int64_t* field_offsets,
                         const int64_t* field_vocab, int n_fields,
                         int64_t batch, int64_t rows_per_rank, int world,
                         int64_t cap, int32_t* send, int32_t* slot_of,
                         void* workspace, int* err_flag, int* overflow_flag,
                         rs_stream_t stream);
int rs_shard_dedup_grad(const float* grad, int64_t grad_stride, int n_fields,
                        int k, int64_t batch, int world, const int32_t* slot_of,
                        void* workspace, float* dst, rs_stream_t stream);

/* Sharded DeepFM backward (ShardedDeepFM.train_step): rs_scatter_rows
 * writes lookup j = b*n_fields + c's gradient row src[b*src_stride + c*k ..]
 * into dst[slot_of[j]] (slot_of < 0 skipped) — the row-exchange layout, so
 * the reverse all-to-all returns every owner the dL/drow of the rows it
 * served, aligned with its received row ids (rs_embedding_sgd on those ids
 * then sums duplicates in record order).                                   */
int rs_scatter_rows(const float* src, int64_t src_stride, int n_fields, int k,
                    const int32_t* slot_of, int64_t batch, float* dst,
                    rs_stream_t stream);
int rs_shard_row_route(const void* ids, int id_kind, int64_t id_stride,
                       const int64_t* field_offsets, const int64_t* field_vocab,
                       int n_fields, int64_t batch, int64_t rows_per_rank,
                       int world, const int32_t* owner_fields, int slot_stride,
                       int32_t* send, int32_t* slot_of, int* err_flag,
                       rs_stream_t stream);
int rs_shard_owner_fm(const int32_t* local_rows, int64_t rec_stride,
                      int field_lo, int n_owned, const float* shard,
                      int64_t shard_rows, int nd, int n_fields, int k,
                      const float* prepared, int kfm, float* partial,
                      int64_t partial_stride, int64_t n_pairs, int* err_flag,
                      rs_stream_t stream);
int rs_shard_fm_combine(const float* partials, int64_t partial_stride,
                        int world, int64_t batch,
                        const float* dense, int64_t dense_stride, int nd,
                        int n_fields, int k, const float* prepared,
                        const float* w0, int kfm, float* logit,
                        rs_stream_t stream);

/* Sharded FM training (sharded.py ShardedEmbeddingFM.train_step;
 * utils/compile_fit.py:9-15 on the FM logit, data parallel over the ranks):
 *  rs_shard_fm_combine_grad: rs_shard_fm_combine that also writes, per
 *   sample, the record gs[b] = [s_0 .. s_{kfm-1} | g] (gs_stride floats
 *   apart; s = x @ v over the whole sample, g = (sigmoid(logit) - label) *
 *   grad_scale, grad_scale = 1 / global batch) and the BCE loss (optional).
 *  rs_shard_owner_fm_grad: owner side of the backward.  recv = the forward's
 *   received row-id records (n_pairs of rec_stride words, requester-major),
 *   gs = every requester's [s | g] records in the same pair order (an
 *   all-gather).  For the owned fields field_lo .. +n_owned: rows_ws [n_pairs,
 *   n_owned*k] = the rows (absent -> 0); drows [n_pairs, n_owned*k] =
 *   dL/drow = g (w1_e + v_e . s - x_e |v_e|^2); dw1 [n_owned*k] and dv
 *   [n_owned*k, kfm] = this owner's part of the FM parameter gradients of
 *   those columns (fixed-order trees; summed over owners by an all-reduce).
 *   w1 / v are the WHOLE model's [d, 1] / [d, kfm].  The row update is then
 *   rs_embedding_sgd on recv (ids = local rows, -1 skipped) and drows.     */
int rs_shard_fm_combine_grad(const float* partials, int64_t partial_stride,
                             int world, int64_t batch, const float* dense,
                             int64_t dense_stride, int nd, int n_fields, int k,
                             const float* prepared, const float* w0, int kfm,
                             const float* labels, float grad_scale,
                             float* logit, float* gs, int64_t gs_stride,
                             float* loss, rs_stream_t stream);
int rs_shard_owner_fm_grad(const int32_t* recv, int64_t rec_stride,
                           int field_lo, int n_owned, const float* shard,
                           int64_t shard_rows, int nd, int k, const float* w1,
                           const float* v, int kfm, const float* gs,
                           int64_t gs_stride, int64_t n_pairs, float* rows_ws,
                           float* drows, float* dw1, float* dv,
                           rs_stream_t stream);

/* One launch per pipelined step (sharded.py pipe_step), run after the
 * step's all-to-all: the owner part of batch t on recv's row-id words
 * (partials -> send's partial words), batch t+1's field route (ids_next ->
 * send's row-id words; ids_next NULL = none) and batch t-1's combine
 * (recv's partial words + dense_prev -> logit_prev; logit_prev NULL = none).
 * recv and send hold world*batch fused records of slot_stride + P words
 * ([row ids | partial]).  The three parts are independent, so one pipelined
 * step is exactly one kernel and one all-to-all.                           */
int rs_shard_fm_pipe(const int32_t* recv, int field_lo, int n_owned,
                     const float* shard, int64_t shard_rows,
                     const float* dense_prev, int64_t dense_stride,
                     float* logit_prev, const void* ids_next, int id_kind,
                     int64_t id_stride, const int64_t* field_offsets,
                     const int64_t* field_vocab, int64_t rows_per_rank,
                     const int32_t* owner_fields, int slot_stride,
                     int32_t* send, int world, int64_t batch, int nd,
                     int n_fields, int k, const float* prepared,
                     const float* w0, int kfm, int* err_flag,
                     rs_stream_t stream);

/* The TWO-DEEP pipelined step with the peer-mapped exchange inside the
 * launch (sharded.py pipe2_step; replaces, for the step, the all-to-all
 * torch.distributed would run before rs_shard_fm_pipe — the lookup sharded is
 * EmbedLayer.call, layer/core.py:273-280).  Launch t = exchange of batch t+1
 * (if `exchange`: this rank's send slot `xsend` = [world][batch] records of
 * [row ids of t+1 | partials of t-1] copied into slot `xslot` of every
 * peer's two-slot mailbox, rs_peer_a2a's ready / full protocol, one step of
 * `peer_state`) | combine of batch t-2 (logit_prev) | owner partials of batch
 * t | field route of batch t+2 (ids_next), the three pipe parts reading
 * `recv` (= this rank's mailbox slot t % 2) and writing `send` (= send slot
 * t % 2).  mailboxes: device array [world] of two-slot mailboxes
 * (rs_peer_mailbox_bytes(world, 2 * batch * R * 4), R = slot_stride +
 * rs_fm_partial_width(kfm)); the launch ends when every peer's block of this
 * step is in this rank's mailbox.  A bounded wait that gives up sets
 * RS_FLAG_TIMEOUT in xerr.  kfm <= 15, <= 32 owned fields, batch * R * 4 a
 * multiple of 16 (else RS_ERR_UNSUPPORTED / RS_ERR_ARG).                    */
int rs_shard_fm_pipe_peer(const int32_t* recv, int32_t* send,
                          const int32_t* xsend, int xslot, int exchange,
                          int field_lo, int n_owned, const float* shard,
                          int64_t shard_rows, const float* dense_prev,
                          int64_t dense_stride, float* logit_prev,
                          const void* ids_next, int id_kind, int64_t id_stride,
                          const int64_t* field_offsets,
                          const int64_t* field_vocab, int64_t rows_per_rank,
                          const int32_t* owner_fields, int slot_stride,
                          int world, int64_t batch, int nd, int n_fields,
                          int k, const float* prepared, const float* w0,
                          int kfm, int* err_flag, void* const* mailboxes,
                          int rank, void* peer_state, int chunks,
                          int64_t spin_limit, int* xerr, rs_stream_t stream);

/* S consecutive batch requests in ONE launch (the headline hot path served
 * back to back: EmbedLayer + concat + FMLayer, layer/core.py:273-280,
 * layer/interaction.py:106-114, per batch as rs_embed_fm_fwd_hm computes it):
 * batch s (s < n_batches) has `batch` samples (the last one last_batch), its
 * ids at ids + s * ids_batch_stride elements (rows id_stride apart), dense at
 * dense + s * dense_batch_stride floats, logits written at logit + s *
 * logit_batch_stride.  Every batch's logits are bit-identical to
 * rs_embed_fm_fwd_hm on that batch alone (same kernel body and tiles).
 * Shapes of the kernarg-metadata kernel only: k in {4, 8, 16}, kfm <= 15,
 * 1..32 fields (host metadata), nd <= 64, int32 / int64 ids, batch <= 8192;
 * min_blocks = 1 or 2 (RS_ERR_ARG otherwise).  Both values run the same
 * kernel: the value was once the second __launch_bounds__ argument, which is
 * a minimum of waves per EU, not of workgroups per CU, and a 1,024-thread
 * workgroup already places 4 waves on every SIMD, so the two builds were
 * identical code.  Timing one against the other measures run-to-run noise. */
int rs_embed_fm_fwd_hm_stream(const void* ids, int id_kind, int64_t id_stride,
                              int64_t ids_batch_stride, const float* dense,
                              int64_t dense_stride, int64_t dense_batch_stride,
                              int nd, const float* table,
                              const int64_t* field_offsets_host,
                              const int64_t* field_vocab_host, int n_fields,
                              int k, const float* prepared, const float* w0,
                              int kfm, float* logit,
                              int64_t logit_batch_stride, int64_t batch,
                              int n_batches, int64_t last_batch,
                              int min_blocks, int* err_flag,
                              rs_stream_t stream);

/* FM over pre-gathered rows (sharded path): emb is [B, F*k] in x order.     */
int rs_rows_fm_fwd(const float* emb, const float* dense, int64_t dense_stride,
                   int nd, int n_fields, int k, const float* prepared,
                   const float* w0, int kfm, float* logit, int64_t batch,
                   rs_stream_t stream);

/* ---- FNN (model/fnn.py:13-67): sigmoid(DNNLayer(x (.) v)) on the compact
 * batch (dense [B, nd], ids [B, F], field_offsets / field_vocab as
 * rs_fm_onehot_fwd), without the dense [B, n*k] input.  Sample b has A = nd +
 * F active features: dense feature j is row j with value dense[b, j], field
 * c is row nd + field_offsets[c] + id(b, c) with value 1.  With the first
 * Dense kernel W1 [n*k, H1] viewed as [n, k, H1] (model/fnn.py:53-57),
 *   z1[b, :] = b1 + sum_a x_a * (v[f_a, :] @ W1[f_a]).
 * An id outside [0, vocab) (or a row past n_rows) sets RS_FLAG_BAD_ID and
 * contributes nothing.  Every offset into W1 / P is int64.  No allocation,
 * no synchronisation: stream-ordered and graph-capturable.
 *
 * rs_fnn_project: P[f, :] = v[f, :] @ W1[f] ([n_rows, H1]; j in order), one
 *  streaming pass over W1 — the inference weight image.
 * rs_fnn_first_layer_fwd: out[b, :] = act(b1 + sum_a x_a P[f_a]) ([B, H1],
 *  rows out_stride apart; act RS_ACT_NONE / RELU / SIGMOID), dense features
 *  first and then the fields, in order.  Any H1.
 * rs_fnn_ok: 1 when rs_fnn_fwd runs a DNN of n_layers Dense layers (the
 *  gathered first one included) with output widths dims[0 .. n_layers-1] and
 *  activations acts[0 .. n_layers-1]: 2..9 layers, dims[n_layers-1] == 1,
 *  RS_ACT_NONE / RELU / SIGMOID, and the fused tower's geometry (padded
 *  widths <= 1024, LDS <= 160 KiB).
 * rs_fnn_fwd: y[b] = sigmoid(DNN(x (.) v)) in one launch: a1 as
 *  rs_fnn_first_layer_fwd computes it (bit-identical), staged in the input
 *  tile of the fused tower, then layers 1.. from `prepared` = rs_mlp_prepare
 *  of those layers (dims[0 .. n_layers-1]).  A shape rs_fnn_ok refuses is
 *  RS_ERR_ARG and launches nothing.                                         */
int rs_fnn_project(const float* v, const float* W1, int64_t n_rows, int k,
                   int H1, float* P, rs_stream_t stream);
int rs_fnn_first_layer_fwd(const void* ids, int id_kind, int64_t id_stride,
                           const float* dense, int64_t dense_stride, int nd,
                           const int64_t* field_offsets,
                           const int64_t* field_vocab, int n_fields,
                           const float* P, int64_t n_rows, int H1,
                           const float* b1, int act, float* out,
                           int64_t out_stride, int64_t batch, int* err_flag,
                           rs_stream_t stream);
int rs_fnn_ok(int n_layers, const int* dims, const int* acts);
int rs_fnn_fwd(const void* ids, int id_kind, int64_t id_stride,
               const float* dense, int64_t dense_stride, int nd,
               const int64_t* field_offsets, const int64_t* field_vocab,
               int n_fields, const float* P, int64_t n_rows, const float* b1,
               int n_layers, const int* dims, const int* acts,
               const float* prepared, float* y, int64_t y_stride,
               int64_t batch, int* err_flag, rs_stream_t stream);

/* FNN stage 2 (the second fit of model/fnn.py:56-63 trains the DNN only; v
 * is a constant).  W1 moves every step, so there is no P: the B*A lookups
 * are sorted once by row (stable radix sort) into `workspace`
 * (rs_fnn_train_workspace_size bytes: O(B*A) + [U, H1] floats for U <=
 * min(B*A, n_rows) distinct rows), and the sort serves both entries.
 * rs_fnn_train_fwd: per distinct row Pu[u] = v[f_u] @ W1[f_u] (a touched
 *  slab is read once however many samples share it), then out[b, :] =
 *  act(b1 + sum_a x_a Pu[slot(b, a)]).
 * rs_fnn_w1_sgd (same shape arguments and the workspace rs_fnn_train_fwd
 *  left): dz1[b, c] = d_a1[b, c] * (mult ? mult[b, c] : 1) where mask is null
 *  or mask[b, c] > 0, else 0 ([B, H1] contiguous; may alias d_a1 when
 *  d_stride == H1); per distinct row g_f = sum over its lookups, in lookup
 *  order, of x * dz1[b] (chunk pieces added in chunk order: no float
 *  atomics, bit-identical run to run); g_out (optional) receives g_f by
 *  ascending row, [U, H1]; W1 (optional) is updated in place, W1[f][j, :] -=
 *  lr * v[f, j] * g_f — rows no sample touched are never written.          */
int64_t rs_fnn_train_workspace_size(int64_t batch, int nd, int n_fields,
                                    int64_t n_rows, int H1);
int rs_fnn_train_fwd(const void* ids, int id_kind, int64_t id_stride,
                     const float* dense, int64_t dense_stride, int nd,
                     const int64_t* field_offsets, const int64_t* field_vocab,
                     int n_fields, const float* v, const float* W1,
                     int64_t n_rows, int k, int H1, const float* b1, int act,
                     float* out, int64_t out_stride, int64_t batch,
                     void* workspace, int* err_flag, rs_stream_t stream);
int rs_fnn_w1_sgd(const float* d_a1, int64_t d_stride, const float* mult,
                  int64_t mult_stride, const float* mask, int64_t mask_stride,
                  const float* dense, int64_t dense_stride, int nd,
                  int n_fields, const float* v, float* W1, int64_t n_rows,
                  int k, int H1, int64_t batch, float lr, float* dz1,
                  float* g_out, void* workspace, rs_stream_t stream);

/* ------------------------------------------------------ evaluation metrics
 * What the reference's scripts print after training: accuracy_score(y_test,
 * [p > 0.5]) (model/fm.py:38, deepFM.py:51, dcn.py:50, din.py:116, pnn.py:89,
 * fnn.py:70-71; metrics=['accuracy'] in utils/compile_fit.py:13), plus the
 * log-loss Keras reports and the ROC AUC two of the scripts name.  Stream-
 * ordered, graph-capturable, no allocation, no synchronisation; n < 2^31 (the
 * size queries answer -1 and the entries RS_ERR_ARG beyond, before any device
 * work); n == 0 is allowed.
 *
 * rs_binary_metrics: pred [n] probabilities (pred_stride floats apart),
 *  labels [n].  result: 8 words of 8 bytes —
 *   0 n            int64
 *   1 n_pos        int64   labels == 1
 *   2 n_correct    int64   (p > 0.5) == (y == 1): Keras binary_accuracy
 *   3 loss_sum     fp64    sum of -(y log(q + eps) + (1 - y) log(1 - q + eps)),
 *                          q = clip(p, eps, 1 - eps), eps = 1e-7, every
 *                          operand promoted to fp64 first (rs_bce_prob_grad's
 *                          form without the fp32 log error)
 *   4 n_bad_label  int64   labels that are neither 0.0 nor 1.0
 *   5 n_nan_pred   int64   NaN predictions (they add nothing to loss_sum)
 *   6, 7           reserved (0)
 *  accumulate != 0 adds into result (which then must hold an earlier result
 *  or zeros) instead of overwriting it.  Sums go workgroup partials -> one
 *  workgroup, in a fixed order: bit-identical run to run.  workspace:
 *  rs_binary_metrics_workspace_size(n) bytes.
 *
 * rs_auc: exact tie-aware ROC AUC of any finite fp32 scores (logits too);
 *  -0.0 ties with +0.0, +-inf are the extremes.  A stable 32-bit radix sort of
 *  (order-preserving key, sample), scans of the positives and of the tie-run
 *  heads, and one thread per tie run adding p_r (2 below_r + n_r) into an
 *  int64 (U2: twice the number of correctly ordered (positive, negative)
 *  pairs, a tied pair counting half); auc = U2 / (2 P Q), NaN when P Q == 0.
 *  group_ids non-null (group_kind RS_ID_I32 / RS_ID_I64, 0 <= id < n_groups;
 *  any other id sets RS_FLAG_BAD_ID in word 6 and is read as group 0): also
 *  gauc = sum_g size_g AUC_g / sum_g size_g over the groups that hold both
 *  classes (impression-weighted, the DIN paper's), from a second stable sort
 *  by group id.  result: 16 words of 8 bytes —
 *   0 n  1 P  2 Q  3 U2            int64
 *   4 auc                          fp64
 *   5 n_nan_score  6 rs_flag bits  7 n_bad_label    int64
 *   8 gauc                         fp64 (NaN without groups / no group used)
 *   9 groups_used  10 impressions_used              int64
 *   11..15                         reserved (0)
 *  With n_nan_score or n_bad_label non-zero the other words mean nothing.
 *  workspace: rs_auc_workspace_size(n, n_groups) bytes (n_groups = 0: no
 *  group ids).  Integer atomics only: bit-identical run to run.            */
int64_t rs_binary_metrics_workspace_size(int64_t n);
int rs_binary_metrics(const float* pred, int64_t pred_stride,
                      const float* labels, int64_t n, int accumulate,
                      void* result, void* workspace, rs_stream_t stream);
int64_t rs_auc_workspace_size(int64_t n, int64_t n_groups);
int rs_auc(const float* scores, int64_t score_stride, const float* labels,
           const void* group_ids, int group_kind, int64_t n_groups, int64_t n,
           void* result, void* workspace, rs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RS_CAPI_H */
