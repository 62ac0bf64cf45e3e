/*
 * polyphemus_hip.h — C ABI of libpolyphemus_hip.so: the MI355X (gfx950) kernels of
 * the Polyphemus graph-VAE hot path.
 *
 * The reference has no FFI of its own (it is pure Python over torch /
 * torch_geometric / torch_scatter); the drop-in boundary is the
 * `nn.Module` surface of `model.VAE`.  Each entry point below replaces the
 * chain of ATen / torch_scatter kernels that one stretch of the reference's
 * Python launches today; the stretch is cited as `file:line` into the
 * reference tree.  The Python mirror (`polyphemus_amd/model.py`) binds these
 * with ctypes; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions (all entry points):
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer owned by
 *     the caller (PyTorch); the library never allocates, frees or synchronises;
 *   - work is enqueued on the caller's `stream` (graph-capturable);
 *   - floats are fp32, row-major, contiguous unless a leading dimension is given;
 *     indices are int32 unless stated;
 *   - return value: 0 = PM_OK, <0 = error (PM_E_*); no exceptions cross the ABI.
 */
#ifndef POLYPHEMUS_HIP_H
#define POLYPHEMUS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* pm_stream_t; /* hipStream_t */

enum {
  PM_OK = 0,
  PM_E_INVALID = -1, /* bad argument (shape, alignment, null pointer) */
  PM_E_LAUNCH = -2,  /* hipGetLastError() != hipSuccess after a launch */
  PM_E_UNSUPPORTED = -3
};

enum { PM_N_REL = 6, PM_N_DIST = 32, PM_N_SLOTS = 15, PM_N_PITCH = 131, PM_N_DUR = 99, PM_N_TOK = 230 };

/* Library / device identification (host only, no GPU needed).  pm_abi_version() returns the PM_ABI_VERSION the library
 * was built with; a host must refuse a library whose version differs from the header it was compiled against (struct
 * layouts — PmBatch, PmGemmDesc, PmVaeLayout —, argument lists and the dropout stream are part of the version).
 *   1: round 1.  2: round 2 (PmBatch.ce_scale, pm_attnpool_bwd +2 arguments, one hash per four channels in the dropout
 *   stream).  3: round 3 (d = 512 in the gcl / linear entry points, pm_gcl_forward_from_planes).
 *   4: round 3, second half (PmGemmDesc.a_colsum — the bias gradient riding in a weight-gradient GEMM —, pm_unembed_ce's
 *   w_planes argument, PM_PLAN_TRK_CNT grown to 32 + 4 W ints by the tile schedule, pm_unembed_dh, pm_bn_small_*,
 *   pm_rows_tn_weight_grad, pm_gcl_tile_order / pm_row_tile_order, pm_vae_step_reload_switches).
 *   5: round 4 (pm_set_deterministic / pm_get_deterministic; plan scratch field grown; PmVaeLayout.flags / .dropout — the
 *   C++ step covers batch_norm = False and cfg.dropout —; pm_vae_step_info writes 16 ints; pm_relu_bwd_planes;
 *   pm_vae_step_backward_encoder_heads, pm_vae_step_join_decoder_grads; pm_head_chain — the latter removed again in ABI 8).
 *   6: round 4, second half (pm_gcl_input_grad_bn / PmBnBwd, pm_bn_bwd_sums: the norm backward inside the input gradient;
 *   pm_chord_pad_vec, pm_chord_tables_fwd, pm_chord_sum_fwd / _bwd, pm_chord_tables_bwd_w / _x: the chord encoder as table algebra).
 *   7: round 5 (the fp16 pair operand format: PmH2, pm_absmax, pm_split_planes_frag_h2, pm_gcl_forward_fused_h2,
 *   pm_gcl_input_grad_bn_h2, pm_gcl_weight_grad_fused_h2; PmNormSums.absmax_out; pm_bn_apply_fused_absmax; pm_vae_step_set_output_grads: the drop-in module's
 *   `model(graph)` + autograd runs the C++ step; pm_vae_step_saved, pm_bn_relu_decisions: parity introspection; pm_batch_flags; pm_unembed_bias_grads; pm_deterministic_faults).
 *   8: round 6 (pm_bar_aggregate_fwd / _bwd: bar-resident aggregation of dense graphs; pm_gcl_forward_from_planes_h2: the dense
 *   route's product in the fp16 pair format; pm_h2_clamp_events: saturation counter of the pair format; PmBatch.flags bit 3 and
 *   pm_vae_step_output_views: the drop-in module's outputs and gradients as views of the arena;
 *   pm_unembed_row_lists / pm_unembed_ce_rows / pm_unembed_dh_rows: the decoder head without its PAD-target rows;
 *   pm_unembed_dw: the three un-embedding weight gradients in one launch).
 *   9: the guarded optimizer step (pm_h2_clamp_init, pm_overflow_snapshot, pm_overflow_poison, pm_grad_nonfinite_check,
 *   pm_adam_step_guarded, pm_adam_bias_scalars; the PM_OVF_* status layout).  Additive, same version: the training
 *   accuracies (pm_vae_step_set_metrics, pm_unembed_ce_metrics, pm_unembed_ce_rows_metrics, pm_content_accuracy_slots,
 *   pm_train_metric_counts; no existing struct or argument list changed); gradient clipping by the global norm
 *   (pm_grad_sumsq, pm_grad_nonfinite_check_sumsq, pm_grad_clip_finish, pm_adam_step_clipped; the PM_CLIP_* layout); the
 *   exponential moving average of the parameters (pm_adam_step_ema, pm_buffer_swap); sampled generation
 *   (pm_sample_tokens, pm_mtp_from_tokens, pm_sample_hash); chord-aware sampling (pm_sample_chords, pm_node_tracks; the
 *   PmChordRules struct); structure sampling (pm_sample_structure; the PmStructureRules struct); note events
 *   (pm_notes_from_tokens); the GCL self block without its round trip (pm_gcl_forward_fused_sel / _sel_h2,
 *   pm_gcl_weight_grad_fused_x / _x_h2: new entry points, no existing argument list changed); harmony (pm_node_cells,
 *   pm_sample_chords_at, pm_note_chroma); the resident data set (pm_dataset_pack_count, pm_dataset_pack_rows,
 *   pm_dataset_gather). */
#define PM_ABI_VERSION 9
int pm_abi_version(void);
const char* pm_build_info(void);

/* Deterministic mode (environment PM_DETERMINISTIC=1 at first use, or pm_set_deterministic).  The reference's CPU step
 * is reproducible run to run (training.py:137-166 on ATen's CPU kernels); the HIP step by default is not, because sums
 * across workgroups (split-K slices of the head products, column statistics of the norms, weight / bias / table
 * gradients) are float atomics whose order follows the hardware's scheduling.  With the mode on, every launch that
 * contains such atomics orders them by a gate (workgroups take turns in dispatch order, csrc/common.h) and the kernels
 * whose workgroups race on an LDS table run one wave per workgroup: two runs of a step on the same inputs are then
 * BIT-IDENTICAL in outputs, losses and gradients (tests/test_deterministic_gpu.py).  Slower (serialised epilogues):
 * for parity tests and debugging.  Host calls, no GPU work. */
int pm_set_deterministic(int32_t on);
int pm_get_deterministic(void);
/* Faults of the mode since the library was loaded (synchronises the device; < 0: could not be read): gates that could not be set
 * up (the launch ran un-gated) + waves that gave up waiting for their turn after 4 s and went ahead unordered.  0 = every gated
 * launch so far was ordered.  While the mode is on the step keeps every launch on the caller's stream (two gated kernels on two
 * streams could starve each other's turns). */
int pm_deterministic_faults(void);
/* Saturation events of the fp16 pair operand format (PmH2 below): the threads of the kernels that split an fp32 tensor into
 * scaled fp16 hi + lo planes (pm_gcl_input_grad_bn_h2, pm_bn_bwd_fused_h2, pm_split_planes_frag_h2) whose value exceeded
 * +-65504 after scaling and was cut — the |max| BOUND the power-of-two scale is taken from was too small by more than 2^3 (the
 * dh bound holds for standardised values |xhat| <= 14; a near-constant BatchNorm column reaches sqrt(N)).  Counted since the
 * library was loaded or since the last call with reset != 0 (synchronises the device; < 0: could not be read).  0 = no gradient
 * was clipped; the parity tests assert it. */
int pm_h2_clamp_events(int32_t reset);
/* Creates the device word of pm_h2_clamp_events (hipMalloc + a synchronous hipMemset) if this device has none yet.  A host
 * calls it once when it sets a model up, so that no launch path is the first to touch the word (the guarded step's
 * pm_overflow_snapshot / pm_overflow_poison refuse to run without it).  0 = the word exists. */
int pm_h2_clamp_init(void);

/* ------------------------------------------------------------------ graph plan
 * Replaces the per-layer boolean-mask edge selection `edge_index[:, edge_type == i]`
 * (model.py:30-38,104-105, 96 times per forward) and the host syncs of
 * `torch.unique(distinct_bars)` (model.py:543) and `batch[-1].item()` (PyG
 * GlobalAttention, model.py:409) by ONE device-side pass per batch:
 * CSR by (dst, relation), CSC by src, per-edge 1/in-degree, bar offsets,
 * drum / non-drum node lists, token histograms.  All integer work, bit-exact.
 *
 * The plan lives in one caller-allocated int32 buffer; `pm_plan_layout` returns the
 * field offsets (in int32 elements) so the host can slice views of it. */
enum {
  PM_PLAN_ROWPTR = 0,   /* [N*6+1] CSR offsets, key = dst*6 + relation            */
  PM_PLAN_CSR_SRC,      /* [E] source node of the edge at this CSR slot           */
  PM_PLAN_CSR_DIST,     /* [E] timestep distance 0..31                            */
  PM_PLAN_CSR_EID,      /* [E] position of the edge in the input edge_index       */
  PM_PLAN_COLPTR,       /* [N+1] CSC offsets, key = src                           */
  PM_PLAN_CSC_DST,      /* [E]                                                    */
  PM_PLAN_CSC_RELDIST,  /* [E] relation | distance << 8                           */
  PM_PLAN_CSC_EID,      /* [E]                                                    */
  PM_PLAN_CSC_INVCNT,   /* [E] float bits: 1 / max(#in-edges of (dst, relation),1) */
  PM_PLAN_NODE_BAR,     /* [N] distinct bar id = bars + n_bars*batch (model.py:403) */
  PM_PLAN_BAR_PTR,      /* [G+1] node offsets of each bar                         */
  PM_PLAN_GROUP_LIST,   /* [2N] drum nodes (ascending) in [0,n_drum); non-drum nodes in [N, N+n_non_drum) */
  PM_PLAN_GROUP_CNT,    /* [4] {n_drum, n_non_drum, 15*n_drum, 15*n_non_drum}     */
  PM_PLAN_TOK_HIST,     /* [4][131] token counts over slots 1..15:
                           0 drum pitch, 1 non-drum pitch, 2 drum dur, 3 non-drum dur */
  PM_PLAN_ROW_LIST,     /* [2*15N] (node, slot) rows = node*15 + slot of the drum nodes in [0, 15 n_drum),
                           of the non-drum nodes from 15N on: row maps of the un-embedding GEMMs */
  PM_PLAN_NODE_TREL,    /* [N] the track relation (0..3) that has in-edges at the node (see pm_segreduce_fwd) */
  PM_PLAN_TRK_LIST,     /* [4N] nodes grouped by that relation (group t at offset t*N), inside a group sorted by
                           class (receives onset edges, receives next edges) in the order (0,0) (1,0) (1,1) (0,1) */
  PM_PLAN_TRK_CNT,      /* [32 + 4 W] {4 group sizes, #nodes with in-edges of more than one track relation, 0,0,0,
                           then 5 class boundaries b0..b4 per group at [8 + 5t + k]: rows [b1,b3) of the list
                           receive onset edges, rows [b2,b4) receive next edges}; from [32] on the tile schedule of
                           the GCL products, (group, first row, rows, 0) for each of the W workgroups of a launch
                           (pm_gcl_tile_order gives the same from a host copy of the first 32 ints) */
  PM_PLAN_SCRATCH,      /* cursors + scan partials                                */
  PM_PLAN_NFIELDS
};
int pm_plan_layout(int32_t N, int32_t E, int32_t G, int64_t* offsets /* [PM_PLAN_NFIELDS+1] */);
int pm_plan_build(const int64_t* edge_index /* [2,E] row0=src,row1=dst (data.py:173) */,
                  const int32_t* edge_type /* [E] 0..5 */, const int32_t* edge_dist /* [E] 0..31 */,
                  const int64_t* bars /* [N] */, const int64_t* batch /* [N] */,
                  const uint8_t* is_drum /* [N] */, const int32_t* tokens /* [N,16,2] */,
                  int32_t n_bars, int32_t n_slots /* active token slots S, 1..15 (see below); 15 = all */,
                  int32_t N, int32_t E, int32_t G, int32_t* plan, pm_stream_t stream);
/* HOST function (no GPU): the schedule of the GCL products over the plan's (track group, 64-row tile) list — the
 * kernels keep one workgroup per CU and a tile costs 2-4 blocks of K, so workgroup b of XCD b % 8 takes the XCD's
 * share of the 4-block tiles first, then of the 3-block, then of the 2-block tiles (csrc/tile_order.h).
 * With 257..264 tiles (one or a few more than the 256 CUs) an XCD that has a tile too many runs one of its cheapest
 * tiles as two 32-row halves behind two others, which keeps the launch as long as its heaviest tile.
 * trk_cnt_host: a host copy of the plan's PM_PLAN_TRK_CNT field [32]; out [3 * cap]: (group, first row of the group's
 * list, rows = 64 | 32) of workgroup b or (-1, -1, 0); returns the number of workgroups a launch for N nodes has. */
int pm_gcl_tile_order(const int32_t* trk_cnt_host, int32_t use_classes, int32_t N, int32_t* out, int32_t cap);
/* ... and of the uniform 64-row tiles of the chord products (pm_rows_times_weight*): out [2 * cap]: (first row, rows =
 * 64 | 32) of workgroup b or (-1, 0); returns the number of workgroups a launch over M rows has. */
int pm_row_tile_order(int32_t M, int32_t* out, int32_t cap);
/* Active slots: slot s >= S holds the PAD token in EVERY node of the batch (S = longest chord + EOS, known
 * to the host that built the batch).  PAD rows carry no loss (ignore_index) and an identical embedding, so the
 * token-level tensors of the fused step are [N, S, .] instead of [N, 15, .]; results are unchanged. */
/* Reference-format inputs -> compact ids (the reference feeds one-hots, data.py:179-182,235-268). */
int pm_edge_attrs_to_ids(const float* edge_attrs /* [E,33] */, int32_t E, int32_t* edge_type,
                         int32_t* edge_dist, pm_stream_t stream);
int pm_tokens_from_onehot(const float* c_tensor /* [N,16,230] */, int32_t N, int32_t* tokens /* [N,16,2] */,
                          pm_stream_t stream);
/* The host-known facts of a batch that does not carry them (a foreign PyG batch: PmBatch.n_slots and flags bit 0):
 * out[0] = last token slot 1..15 holding a non-PAD token in some node (0: none), out[1] != 0: some node receives track
 * edges of more than one track relation (the compact GCL does not apply), out[2] != 0: a token id, edge type or node id is
 * out of range.  `seen` [N] and `out` [3] are caller-zeroed device ints; the caller reads `out` (its one host sync). */
int pm_batch_flags(const int32_t* tokens /* [N,16,2] */, const int64_t* edge_index /* [2,E] */, const int32_t* edge_type,
                   int32_t N, int32_t E, int32_t* seen, int32_t* out, pm_stream_t stream);

/* ------------------------------------------------------------------ device-side graph construction
 * `graph_from_tensor` + the PyG collate of the reference (data.py:24-204) for a whole batch of bars on
 * the device: same node numbering (active cells in (track, timestep) order), same edge order (per bar: track edges per
 * track forward-then-inverse, onset edges per timestep forward-then-inverse, next edges forward only; self loop for an
 * edgeless bar), cell [0,0] of an empty bar switched on in place.  Two calls, the caller sizes the outputs in between
 * (totals[0] = N, totals[1] = E; the only host read):
 *   pm_graph_count: per-bar node / edge counts and their exclusive scans node_ptr / edge_ptr [G+1];
 *   pm_graph_emit : edge_index [2,E] (int64, batch-global node ids), edge_type / edge_dist [E], bars / batch [N]
 *                   (bar index inside the sample, sample index), is_drum [N], node_cell [N] = (g*4 + track)*32 + timestep
 *                   (gathers per-cell payloads such as the token grid). */
int pm_graph_count(float* s_tensor /* [G,4,32] 0/1, empty bars fixed in place */, int32_t G, int32_t* bar_nodes /* [G] */,
                   int32_t* bar_edges /* [G] */, int32_t* node_ptr /* [G+1] */, int32_t* edge_ptr /* [G+1] */,
                   int32_t* totals /* [2] */, pm_stream_t stream);
int pm_graph_emit(float* s_tensor, int32_t G, int32_t n_bars, const int32_t* node_ptr, const int32_t* edge_ptr, int64_t N,
                  int64_t E, int64_t* edge_index, int32_t* edge_type, int32_t* edge_dist, int64_t* bars, int64_t* batch,
                  uint8_t* is_drum, int32_t* node_cell, pm_stream_t stream);

/* Generation helpers, no host synchronisation:
 *   pm_binary_from_logits: `Decoder._binary_from_logits` (model.py:609-623): sigmoid(s_logits) >= thresh, an empty bar
 *                          gets cell [0,0]; written as float 0/1 and / or bytes (either output may be NULL, not both).
 *   pm_mtp_from_logits   : `mtp_from_logits` (utils.py:59-79): mtp [G,4,32,15,230] = the node's logits on active cells
 *                          (nodes numbered in cell order), the hard silence elsewhere (row 0 one-hot pitch EOS = 129,
 *                          rows 1..14 one-hot pitch PAD = 130).  bar_nodes [G] and node_ptr [G+1] are workspaces;
 *                          node_ptr[G] returns the number of active cells, which the caller compares with N (the
 *                          reference raises on a mismatch; the kernel itself writes silence for nodes >= N). */
int pm_binary_from_logits(const float* s_logits /* [G,4,32] */, int32_t G, float thresh, float* s_f32 /* [G,4,32] */,
                          uint8_t* s_u8 /* [G,4,32] */, pm_stream_t stream);
int pm_mtp_from_logits(const float* c_logits /* [N,15,230] */, const float* s_tensor /* [G,4,32] 0/1 */, int32_t G,
                       int64_t N, int32_t* bar_nodes /* [G] */, int32_t* node_ptr /* [G+1] */,
                       float* mtp /* [G,4,32,15,230] */, pm_stream_t stream);

/* ------------------------------------------------------------------ Resident data set
 * A whole data set kept on the device in compact form, and batches gathered from it by index.  Replaces what the reference
 * does per sample, per batch and per epoch on the host: `PolyphemusDataset.__getitem__` opening one `.npz` and re-laying
 * the dense token grid out bar by bar (data.py:218-233), and the random transposition that preprocessing bakes into the
 * files once (preprocess.py:196-205), which a resident set draws afresh for every batch.  Additive, same ABI version.
 *
 * The store of n samples of n_bars bars (1 <= n_bars <= 64):
 *   s_bits   [n, n_bars, 4] uint32  bit t of word (bar, track): cell (track, t) of the bar is active; a bar without an active
 *                                   cell has cell [0,0] (data.py:148-153).
 *   rows     [R, 16, 2] uint8       the token rows (pitch id < 131, duration id < 99) of the active cells of all samples, in
 *                                   the order pm_graph_emit numbers nodes in: (sample, bar, track, step).
 *   cell_ptr [n + 1] int64          the rows of sample i are rows[cell_ptr[i] : cell_ptr[i + 1]].
 *
 * pm_dataset_pack_count (data.py:218-233): a chunk of n samples in the layout the reference's __getitem__ produces,
 *   token_grid int16 [n, n_bars, 4, 32, 16, 2] and s_grid uint8 [n, n_bars, 4, 32] (non-zero = active), becomes s_bits
 *   [n, n_bars, 4], cells [n] (active cells per sample, the empty-bar cell included) and last_slot [n] (the last of the
 *   slots 1..15 that holds a non-PAD pitch or duration in an active cell, 0: none).  status [1], zeroed by the caller, gains
 *   the number of token ids of active cells outside [0, 131) / [0, 99).  One launch, a workgroup per sample.
 * pm_dataset_pack_rows (data.py:218-233): the byte rows of the chunk's active cells, written at rows[row_base + cell_off[i]
 *   + r] for cell r of sample i; cell_off [n + 1] int64 is the exclusive scan of `cells` inside the chunk, row_base the
 *   64-bit row at which the chunk starts and R the rows the buffer holds.  Nothing is written at or beyond row R nor beyond
 *   a sample's span of cell_off.  Ids are cut to their low byte (pm_dataset_pack_count has counted those that do not fit).
 * pm_dataset_gather (data.py:218-233, preprocess.py:196-205): batch entry j < B is sample index[j]; in ONE launch, a
 *   workgroup per entry, s_tensor [B n_bars, 4, 32] fp32 0/1 is expanded from the masks and the entry's rows are widened to
 *   tokens [N, 16, 2] int32 at row out_ptr[j].  out_ptr [B + 1] int32 is the caller's exclusive scan of the entries' cells
 *   (host arithmetic on the counts of pm_dataset_pack_count): no device scan, nothing to read back.  An entry is followed
 *   iff 0 <= index[j] < n and out_ptr[j + 1] - out_ptr[j] equals both cell_ptr's span of the sample and the cells of its
 *   masks, with 0 <= out_ptr[j], out_ptr[j + 1] <= N, 0 <= cell_ptr[i] and cell_ptr[i + 1] <= R.  Any other gets a structure
 *   of zeros and no row and is counted in status [2], zeroed by the caller: [0] indices outside [0, n), [1] spans that do
 *   not match.  No row at or beyond N is written, whatever the inputs hold.  Entries may repeat.
 *   transpose  NULL or [B] int32 semitones: on tracks 1..3 (never the drums) a pitch id <= 127 (not SOS, EOS or PAD) of
 *              entry j becomes clamp(id + transpose[j], 0, 127); durations are untouched.  The caller keeps |shift| <= 127.
 * The only atomics are the status counters.  Per batch 32 B are read and 128 B written per row, 16 B read and 512 B written
 * per bar.
 * PM_E_INVALID (before any launch): a NULL pointer (transpose may be NULL); n < 1, B < 1, N < 1, R < 1, row_base < 0 or
 *   >= R; n_bars outside [1, 64]; 128 n n_bars (pack) or 128 B n_bars (gather) >= 2^31; n (gather) or N >= 2^31; N above
 *   128 B n_bars; R above 2^40; token_grid, rows, s_tensor or tokens not 16-byte aligned, cell_off / cell_ptr not
 *   8-byte aligned, any other pointer but s_grid not 4-byte aligned; an output overlapping any other buffer. */
int pm_dataset_pack_count(const int16_t* token_grid /* [n,n_bars,4,32,16,2] */, const uint8_t* s_grid /* [n,n_bars,4,32] */,
                          int64_t n, int32_t n_bars, uint32_t* s_bits /* [n,n_bars,4] */, int32_t* cells /* [n] */,
                          int32_t* last_slot /* [n] */, int32_t* status /* [1] */, pm_stream_t stream);
int pm_dataset_pack_rows(const int16_t* token_grid /* [n,n_bars,4,32,16,2] */, const uint32_t* s_bits /* [n,n_bars,4] */,
                         const int64_t* cell_off /* [n+1] */, int64_t n, int32_t n_bars, uint8_t* rows /* [R,16,2] */,
                         int64_t row_base, int64_t R, pm_stream_t stream);
int pm_dataset_gather(const uint32_t* s_bits /* [n,n_bars,4] */, const uint8_t* rows /* [R,16,2] */,
                      const int64_t* cell_ptr /* [n+1] */, int64_t n, int32_t n_bars, int64_t R,
                      const int32_t* index /* [B] */, const int32_t* out_ptr /* [B+1] */,
                      const int32_t* transpose /* [B] or NULL */, int32_t B, int64_t N, float* s_tensor /* [B n_bars,4,32] */,
                      int32_t* tokens /* [N,16,2] */, int32_t* status /* [2] */, pm_stream_t stream);

/* ------------------------------------------------------------------ sampled generation
 * No line of the reference stands behind these entries: its `muspy_from_mtp` (utils.py:103-105) takes the arg-max of every
 * (cell, slot, head), so one latent gives one piece.  pm_sample_tokens draws the pitch and the duration token of every
 * (node, slot) row on the device instead (temperature, top-k, nucleus), pm_mtp_from_tokens lays their one-hot rows out as
 * the pianoroll, whose per-head arg-max is then the drawn token: `muspy_from_mtp` is fed unchanged.  Additive, same ABI
 * version.
 *
 * c_logits is [N,15,230] fp32, contiguous; row r = n*15 + slot.  Head 0 (pitch) is the columns [0,131), head 1 (duration)
 * the columns [131,230): V = 131 / 99, a token is a column index inside its head.  Every (row, head) is decided on its own.
 *   rank    : tokens are ordered by raw logit, descending, equal logits by lower index first (exact: no arithmetic).
 *   top_k   : 0 or >= V means off; otherwise the tokens of rank < top_k survive.
 *   top_p   : in (0, 1], 1 means off.  Over the top_k survivors q_i = expf((l_i - max) * inv_T), Z = sum of q_i; a token
 *             survives iff the q-mass of the survivors that outrank it is < top_p * Z.  The top token always survives.  The
 *             order of the summations is the implementation's choice.
 *   draw    : the arg-max over the survivors of l_i * inv_T + g_i in fp32 (a product, then a sum), lowest index on ties;
 *               inv_T = (float)(1.0 / (double)temperature)
 *               g_i   = -logf(-logf(u_i))                     (logf, not a fast variant: the library is built without fast-math)
 *               u_i   = ((h >> 9) + 0.5f) * 2^-23             (exact in fp32, strictly inside (0, 1))
 *               h     = pm_mix32(key(seed, head, r) + token * 0xC2B2AE35u)
 *               key   = pm_mix32(pm_mix32(seed ^ (head + 1u) * 0x9E3779B9u) ^ (r * 0x85EBCA6Bu + 0x27D4EB2Fu))
 *             (pm_mix32 and the key construction are those of the dropout stream, csrc/common.h.)  The stream is a pure
 *             function of (seed, head, row, token): it depends neither on the launch shape nor on the wave that has the row.
 *   temperature == 0: greedy, the arg-max of the raw logits, lowest index on ties, no noise; top_k == 1 gives the same tokens.
 *   non-finite logits: nothing is promised about which token comes out; every token written is in [0, V) and nothing is
 *             written outside `tokens`.
 * pm_sample_tokens: one wave per row, the logits read once, tokens [rows,2] int32 = {pitch, duration} written.
 *   PM_E_INVALID (before any launch): a NULL pointer, rows <= 0 or >= 2^32, temperature < 0 / NaN / inf, top_k < 0, top_p
 *   outside (0, 1] (NaN included).
 * pm_mtp_from_tokens: pm_mtp_from_logits with an active cell holding, per slot, 1.0 at column `pitch` and at column
 *   131 + `duration` and 0 elsewhere (tokens [N,15,2]); a token outside its head's range lights no column of that head.  The
 *   silence of the inactive cells, the workspaces, node_ptr[G] and the argument checks are those of pm_mtp_from_logits.
 * pm_sample_hash: host-callable, h >> 9 of the draw above (the 23 bits u_i is made of). */
int pm_sample_tokens(const float* c_logits /* [rows,230] */, int64_t rows, float temperature, int32_t top_k, float top_p,
                     uint32_t seed, int32_t* tokens /* [rows,2] */, pm_stream_t stream);
int pm_mtp_from_tokens(const int32_t* tokens /* [N,15,2] */, const float* s_tensor /* [G,4,32] 0/1 */, int32_t G, int64_t N,
                       int32_t* bar_nodes /* [G] */, int32_t* node_ptr /* [G+1] */, float* mtp /* [G,4,32,15,230] */,
                       pm_stream_t stream);
uint32_t pm_sample_hash(uint32_t seed, uint32_t row, uint32_t head, uint32_t token);

/* Chord-aware sampling.  The reference reads a cell with `muspy_from_mtp` (utils.py:95-124): it walks the 15 slots in order,
 * stops at the first slot whose pitch or duration is EOS / PAD and skips SOS.  pm_sample_chords draws a cell the way the
 * training data lays one out (notes, one EOS, then PAD), under per-track rules.  Additive, same ABI version.
 *
 * For node n of track t = node_track[n] the slots s = 0..14 are decided in order, from the state count = 0, used = {},
 * ended = false.  Per slot:
 *   ended              : the slot's tokens are (PAD 130, PAD 98).
 *   pitch candidates   : every pitch p < 128 whose pitch_mask[t] bit is set and that is not in `used`, but only while
 *                        count < max_notes[t]; EOS (129) iff count >= min_notes[t] or there is no pitch candidate (the mask
 *                        is exhausted, or count == max_notes[t]); SOS (128) and PAD (130) never.
 *   pitch draw         : the pitch-head token of row r = n*15 + s by the definition above restricted to the candidates: rank,
 *                        top_k, top_p and the Gumbel draw with the same key(seed, head, r) and per-token hash; a column that
 *                        is no candidate is absent (it takes no rank, adds no mass to Z or to an outranking sum and cannot
 *                        win); `max` in q_i is the maximum over the candidates; inv_T comes from temperature[0].  A single
 *                        candidate is taken without a draw.
 *   EOS drawn          : the slot's tokens are (129, 97), ended = true.
 *   otherwise          : the duration head (head 1, same row) is drawn over the candidates 0..95 with temperature[1] (SOS 96,
 *                        EOS 97 and PAD 98 never); the slot's tokens are (p, d), p joins `used`, count += 1.
 * note_count[n] is the final count; max_notes <= 14 makes slot 14 at most the EOS.  The duration head has no say about the
 * end of a chord.  Hence `muspy_from_mtp` on pm_mtp_from_tokens(tokens) yields exactly note_count[n] notes for node n, with
 * distinct allowed pitches; and with the filters off the arg-max runs over a subset with the same fp32 scores, so where
 * pm_sample_tokens (same seed, temperature == temperature[head]) draws a pitch token that is a candidate, or a duration token
 * below 96, the chord's token at that slot is that token.
 *   a temperature of 0 : the arg-max of that head's raw logits over its candidates, lowest index on ties; top_k == 1 gives
 *                        that on both heads.
 *   non-finite logits  : every token is in its head's range, note_count is in [0,14], nothing is written outside the outputs;
 *                        which tokens come out is not promised.
 * pm_sample_chords: one wave per node, at most the rows up to the chord's end (and one more) read; tokens [N,15,2] int32 and
 *   note_count [N] (optional) written.  `rules` is read by the call.  PM_E_INVALID (before any launch): NULL c_logits,
 *   node_track, rules or tokens; N <= 0 or N*15 >= 2^32; a temperature that is negative, NaN or inf; top_k < 0; top_p outside
 *   (0, 1]; a track with min_notes < 0, max_notes outside [1,14] or min_notes > max_notes.
 * pm_node_tracks: node_track[n] = the track index of node n's cell, nodes numbered in cell order as in pm_mtp_from_tokens;
 *   entries n >= the number of active cells are written 0, nothing is written at or beyond N; node_ptr[G] returns the number
 *   of active cells.  The workspaces and the argument checks are those of pm_mtp_from_tokens. */
typedef struct PmChordRules {
  float    temperature[2];   /* [0] pitch head, [1] duration head: finite, >= 0; 0 = arg-max over the candidates of that head */
  int32_t  top_k;            /* as pm_sample_tokens (0 = off), applied to the candidates */
  float    top_p;            /* as pm_sample_tokens, in (0, 1], applied to the candidates */
  int32_t  min_notes[4];     /* per track (Drums, Bass, Guitar, Strings): 0 <= min_notes <= max_notes */
  int32_t  max_notes[4];     /* 1 <= max_notes <= 14 */
  uint32_t pitch_mask[4][4]; /* per track: bit (p & 31) of word (p >> 5) set = MIDI pitch p in [0,128) may be drawn */
} PmChordRules;              /* 112 bytes, a HOST struct: read by the call, passed to the kernel by value */

int pm_sample_chords(const float* c_logits /* [N,15,230] */, const uint8_t* node_track /* [N], values 0..3 */, int64_t N,
                     const PmChordRules* rules, uint32_t seed, int32_t* tokens /* [N,15,2] */,
                     int32_t* note_count /* [N] or NULL */, pm_stream_t stream);
int pm_node_tracks(const float* s_tensor /* [G,4,32] 0/1 */, int32_t G, int64_t N, int32_t* bar_nodes /* [G] ws */,
                   int32_t* node_ptr /* [G+1] ws; node_ptr[G] = active cells */, uint8_t* node_track /* [N] */, pm_stream_t stream);

/* Structure sampling.  The reference decides which of the 4 x 32 (track, timestep) cells of a bar are active by thresholding
 * sigmoid(s_logits) (pm_binary_from_logits): one latent, one rhythm.  pm_sample_structure draws the cells from the model's own
 * probabilities instead, under per-track rules: how many cells of a track may be active, and on which timesteps.  No line of
 * the reference stands behind it.  Additive, same ABI version.
 *
 * s_logits is [G,4,32] fp32, contiguous: bar g, track k (Drums, Bass, Guitar, Strings), timestep t, cell index c = 32k + t.
 * A cell is allowed iff bit t of step_mask[k] is set; a cell that is not allowed is off and takes no rank.
 *   score   : of an allowed cell with logit x, in fp32, one rounding per operation, in exactly this order:
 *               temperature == 0 : score = x - bias[k]                       (no noise)
 *               otherwise        : score = (x - bias[k]) * inv_T + L
 *                 inv_T = (float)(1.0 / (double)temperature)
 *                 L     = logf(u) - logf(1.0f - u)             (logistic noise; 1.0f - u is exact)
 *                 u     = ((h >> 9) + 0.5f) * 2^-23
 *                 h     = pm_mix32(key(seed, head = 2, r = g) + c * 0xC2B2AE35u)
 *             key and pm_mix32 are those of pm_sample_tokens, and pm_sample_hash(seed, g, 2, c) returns h >> 9.  Head 2 keeps
 *             the structure stream apart from the pitch (0) and the duration (1) stream of the same seed.  The stream is a
 *             pure function of (seed, g, c): it depends neither on the launch shape nor on the wave that has the bar.  With
 *             no bound binding a cell is therefore on with probability sigmoid((x - bias[k]) / temperature); the host passes
 *             bias = logit(threshold), so a threshold of 0.5 is a bias of 0.
 *   rank    : within each (bar, track) the allowed cells are ordered by score, descending, equal scores by lower t first.  The
 *             order is a total order on the bits of the score (the score as an unsigned key of the same order, -0 = +0, as
 *             csrc/sample.hip orders logits), so the ranks are a permutation of 0 .. allowed - 1 even when a score is not finite.
 *   on/off  : an allowed cell is on iff rank < min_active[k], or rank < max_active[k] and !(score < 0).  max_active[k] == 0
 *             mutes the track; min_active[k] forces the best cells on whatever their scores.
 *   no empty bar : where this leaves a bar without any cell, the allowed cell with the highest score among the tracks with
 *             max_active > 0 is switched on, the lowest cell index on ties.  (The reference's fake drum hit at [0,0],
 *             model.py:617-621, may be masked or muted here.)
 *   outputs : s_f32 and / or s_u8 [G,4,32] hold 0 / 1 (either may be NULL, not both); track_count [G,4] (optional) holds the
 *             active cells of every (bar, track), counted after the no-empty-bar step.
 *   non-finite logits: every output is 0 or 1, every count is in [min_active, max_active] except for the one cell the
 *             no-empty-bar step may add to a track with min_active == 0, no bar is empty and nothing is written outside the
 *             outputs; which cells come out is not promised.
 * Relation to pm_binary_from_logits: with temperature = 0, bias = 0, bounds 0 .. 32 and full masks a cell is on iff !(x < 0),
 *   there iff !(sigmoid(x) < 0.5).  The two agree wherever |x| >= 1e-6 and the thresholded bar is not empty; they may differ
 *   within a rounding of x = 0 (expf rounds, the comparison with 0 does not) and in the cell an empty bar gets ([0,0] there,
 *   the best-scoring cell here).  They are not bit-identical.
 * pm_sample_structure: one launch, a bar per half-wave, every logit read once, every output written once, no workspace.
 *   `rules` is read by the call.  PM_E_INVALID (before any launch): NULL s_logits or rules, or both s_f32 and s_u8 NULL;
 *   G <= 0; a temperature that is negative, NaN or inf; a bias that is not finite; a track with min_active < 0,
 *   max_active > 32, min_active > max_active or min_active > popcount(step_mask); no track with both max_active > 0 and a
 *   non-zero step_mask. */
typedef struct PmStructureRules {
  float    temperature;      /* finite, >= 0; 0 = no noise */
  float    bias[4];          /* per track: logit(threshold), computed by the host in double */
  int32_t  min_active[4];    /* 0 <= min_active <= max_active */
  int32_t  max_active[4];    /* 0..32; 0 mutes the track */
  uint32_t step_mask[4];     /* bit t set = timestep t of the track may be active */
} PmStructureRules;          /* 68 bytes, a HOST struct: read by the call, passed to the kernel by value */

int pm_sample_structure(const float* s_logits /* [G,4,32] */, int32_t G, const PmStructureRules* rules, uint32_t seed,
                        float* s_f32 /* [G,4,32] or NULL */, uint8_t* s_u8 /* [G,4,32] or NULL */,
                        int32_t* track_count /* [G,4] or NULL */, pm_stream_t stream);

/* ------------------------------------------------------------------ Note events
 * The reference turns a generated pianoroll into notes on the host (`muspy_from_mtp`, utils.py:83-124): a Python loop over
 * every (track, time, slot) with two arg-maxes and three `.item()` reads each.  pm_notes_from_tokens reads the same notes out
 * of the tokens of sampled generation, on the device, without the pianoroll: the result is exactly
 * muspy_from_mtp(pm_mtp_from_tokens(tokens, s_tensor)[i]) for every piece i.  Additive, same ABI version.
 *
 * s_tensor is [G,4,32] with G = B * n_bars: bar g = i * n_bars + b of piece i, track k, timestep s; the cell's time is
 * t = 32 b + s.  Nodes are numbered in cell order as in pm_node_tracks.  The 15 slots of an active cell are walked in order:
 *   stop   at a pitch of 129 (EOS) or 130 (PAD), or a duration token of 97 (EOS) or 98 (PAD);
 *   skip   a pitch of 128 (SOS);
 *   emit   otherwise the row (t, pitch, min(duration token + 1, 32 n_bars - t)).
 * The reference never tests for a duration SOS (utils.py:114-115 tests the pitch twice), so a duration token of 96 is a note
 * of length 97 before the clamp.  A token outside its head's range reads as 0, the arg-max of the all-zero head that
 * pm_mtp_from_tokens leaves.  An inactive cell emits nothing, nor does a cell whose node index is >= N.
 *   notes     [capacity,3] int32 (time, pitch, duration): the rows of (piece i, track k) are
 *             notes[track_ptr[4i+k] : track_ptr[4i+k+1]], inside that range by time, then by slot — the order in which the
 *             reference appends them.  Rows at M and beyond are not written.
 *   track_ptr [4B+1]; track_ptr[4B] = totals[0] = M, the number of notes; totals[1] = the number of active cells, which the
 *             caller compares with N as for pm_mtp_from_tokens.
 *   scratch   seg_count [4G] and seg_ptr [4G+1] (segment (4i+k) * n_bars + b = one track of one bar), bar_nodes [G] and
 *             node_ptr [G+1] as for pm_node_tracks.
 * Five launches on the stream (cells per bar, their scan, notes per segment, their scan, the rows), no host read, no atomics:
 * two calls on the same inputs write the same bytes.  120 B are read per node and at most 180 B written.
 * PM_E_INVALID (before any launch, so no kernel can write past `notes`): capacity < 15 N; G <= 0, n_bars <= 0 or
 *   G % n_bars != 0; N < 0 or 15 N >= 2^31; G * 128 >= 2^31; a NULL pointer (tokens and notes may be NULL when N == 0); tokens
 *   not 8-byte aligned; any two of the scratch and output buffers overlapping. */
int pm_notes_from_tokens(const int32_t* tokens /* [N,15,2] pitch, duration */, const float* s_tensor /* [G,4,32] 0/1 */,
                         int32_t G, int32_t n_bars, int64_t N, int32_t* seg_count /* [4G] ws */,
                         int32_t* seg_ptr /* [4G+1] ws */, int32_t* bar_nodes /* [G] ws */, int32_t* node_ptr /* [G+1] ws */,
                         int32_t* notes /* [capacity,3] */, int64_t capacity, int32_t* track_ptr /* [4B+1] */,
                         int32_t* totals /* [2]: notes M, active cells */, pm_stream_t stream);

/* ------------------------------------------------------------------ Notes in
 * The inverse of pm_notes_from_tokens: pieces held as note events become the structure tensor and the node tokens the encoder
 * consumes.  The reference does this on the host, one track at a time, while it preprocesses MIDI files (preprocess.py:118-157),
 * and switches cell [0,0] of an empty bar on when it builds the bar graphs (data.py:148-153); pm_tokens_from_notes does both
 * for a batch of pieces on the device.  Additive, same ABI version.
 *
 * notes is [M,3] int32 (time, pitch, duration) and track_ptr [4B+1] int32, as pm_notes_from_tokens writes them: the rows of
 * (piece i, track k) are notes[track_ptr[4i+k] : track_ptr[4i+k+1]].  Contract: track_ptr starts at 0, does not decrease and
 * ends at or below M (rows behind its last entry belong to no track: the notes buffer of pm_notes_from_tokens is sized for
 * the worst case); inside a track's range the times do not decrease and lie in [0, 32 n_bars).  Cell (bar g = i * n_bars + b, track k,
 * timestep s) holds the rows of its track whose time is 32 b + s, in row order:
 *   slots    : slot 0 is (SOS 128, SOS 96); the first 14 rows take the slots 1..14 as (clamp(pitch, 0, 127),
 *              clamp(duration, 1, 96) - 1); later rows are dropped (preprocess.py:136-138); the slot behind the last kept row is
 *              (EOS 129, EOS 97), the rest (PAD 130, PAD 98).
 *   activity : a cell is active iff it holds a row; a bar without an active cell gets cell [0,0] switched on with no note.
 *   s_tensor [G,4,32] fp32 0 / 1, G = B * n_bars; every entry is written.
 *   tokens   [capacity,16,2] int32 (pitch, duration): node n is the n-th active cell in cell order, as in pm_graph_emit and
 *            pm_node_tracks.  Nodes at `capacity` and beyond are not written, nor are rows of `tokens` behind the last node;
 *            min(M + G, 128 G) nodes always suffice for input that keeps the contract.
 *   status   [5]: rows whose time is outside [0, 32 n_bars); rows whose time is above the next row's of the same track;
 *            track_ptr entries that break the contract (entry 0 unless it is 0; a later entry outside [0, M] or below the
 *            entry before it); notes dropped for lack of slots; the number of nodes N.
 *   scratch  PM_NOTES_IN_SCRATCH(B, n_bars) int32.
 * Input that breaks the contract is counted, never followed: every track's range is clamped into [0, M] before a row is read
 * and every cell's rows are found by binary search inside that range, so nothing outside notes[0:M] and track_ptr[0:4B+1] is
 * read; what s_tensor and tokens then hold is still a function of the input alone.  The counts cover the rows inside the
 * clamped ranges.
 * Six launches on the stream (the check, the cells' rows, active cells per bar, their scan, the nodes, the status sums), no
 * host read, no atomics: two calls on the same inputs write the same bytes.  12 B are read per note by the check, and per
 * cell about 4 log2(notes of the track) rows by each of the two search passes; 128 B are written per node and 512 B per bar.
 * PM_E_INVALID (before any launch): a NULL pointer (notes may be NULL when M == 0, tokens when capacity == 0); B <= 0,
 *   n_bars <= 0, M < 0 or capacity < 0; 128 G, 3 M or 32 capacity >= 2^31; a pointer not 4-byte aligned, tokens not 16-byte
 *   aligned; any two buffers overlapping except the two inputs. */
#define PM_NOTES_IN_SCRATCH(B, n_bars) (3 * (int64_t)(B) * (n_bars) + 1 + 12 * (int64_t)(B))
int pm_tokens_from_notes(const int32_t* notes /* [M,3] time, pitch, duration */, const int32_t* track_ptr /* [4B+1] */,
                         int32_t B, int32_t n_bars, int64_t M, float* s_tensor /* [B*n_bars,4,32] */,
                         int32_t* tokens /* [capacity,16,2] */, int64_t capacity,
                         int32_t* scratch /* [PM_NOTES_IN_SCRATCH(B, n_bars)] */, int32_t* status /* [5] */,
                         pm_stream_t stream);

/* ------------------------------------------------------------------ Infill
 * Regenerate chosen tracks, bars and steps of a piece around the notes that are kept: the input's structure and node tokens
 * (pm_tokens_from_notes) are merged with what the model gives for the same latent, under a region mask.  The decoder is not
 * autoregressive, so kept and regenerated cells are independent given z and the bar graph: the merge is two passes over the
 * bar layout, one for the structure before the content decoder runs and one for the tokens after the draw.  Additive, same
 * ABI version.
 *
 * region is uint8 [R,4,32] (0 / non-zero: the model rewrites the cell) in the cell layout of a structure tensor; bar g reads
 * region row g % R.  R is G (a mask per piece and bar) or a divisor of G (R = n_bars: one mask shared by all pieces).
 *
 * pm_infill_structure: a cell is on iff (region ? s_model != 0 : s_in != 0).
 *   s_in     fp32 [G,4,32] 0 / 1, the input's structure as pm_tokens_from_notes wrote it;
 *   s_model  uint8 [G,4,32], what pm_binary_from_logits or pm_sample_structure wrote;
 *   no empty bar : where that leaves a bar without a cell, cell [0,0] is switched on (data.py:152-153, the rule
 *            pm_tokens_from_notes and pm_graph_count apply), whether or not [0,0] lies in the region; bar_forced[g] = 1
 *            there, else 0;
 *   outputs  s_f32 and / or s_u8 [G,4,32] hold 0 / 1 (either may be NULL, not both); bar_forced int32 [G].
 *   One launch, a bar per half-wave, every input read once, every output written once, no atomics, no LDS, no workspace.
 *   768 B are read per bar (s_in 512, s_model 128, region 128) and up to 644 B written.
 *
 * pm_infill_tokens: the kept cells' tokens go from the input's node numbering into the merged structure's.
 *   s_out    fp32 [G,4,32], the merged structure after the decoder's graph build; its nodes and those of s_in are the active
 *            cells in cell order, as in pm_node_tracks;
 *   tokens_in int32 [N_in,16,2], the input's node tokens (slot 0 = SOS) as pm_tokens_from_notes wrote them;
 *   tokens   int32 [N,15,2], in / out: on entry the drawn tokens of every node of s_out, the form pm_notes_from_tokens reads.
 *   A cell that is on in s_out and
 *     inside the region                  : its row stays as drawn;
 *     outside the region, on in s_in     : tokens[n_out, j] = tokens_in[n_in, j + 1] for j = 0..14 (the SOS slot is dropped);
 *     outside the region, off in s_in    : (the forced [0,0]) slot 0 is (EOS 129, EOS 97), slots 1..14 are (PAD 130, PAD 98):
 *                                          the chord of a cell without a note (preprocess.py:118-157), which
 *                                          pm_tokens_from_notes gives an empty bar's cell.
 *   Nothing is read at or beyond node N_in and nothing is written at or beyond node N: a mismatch is counted, never followed.
 *   A kept cell whose input node lies at or beyond N_in has no source and takes the chord without a note; a cell whose node
 *   in s_out lies at or beyond N is neither written nor counted as kept.
 *   bar_forced int32 [G] as pm_infill_structure wrote it, or NULL (no bar counted).
 *   status   [5]: active cells of s_out; active cells of s_in; kept nodes; kept nodes without a source; bars forced (the sum
 *            of bar_forced).  Built from per-bar counts in scratch and summed by one wave.
 *   scratch  PM_INFILL_SCRATCH(G) int32: active cells per bar and node_ptr of both structures, two counts per bar.
 *   Six launches on the stream (active cells per bar and their scan for each structure, the rows, the status sums), no host
 *   read, no atomics: two calls on the same inputs write the same bytes.  A row of tokens is 120 B, so rows are 8-byte
 *   aligned, not 16: a kept node is fifteen 8-byte loads and fifteen 8-byte stores, 120 B each way; per bar 1152 B of
 *   structure and region are read by the rows launch and 1024 B by the two counts.
 *
 * PM_E_INVALID (both entries, before any launch): a NULL pointer where one is needed (tokens_in may be NULL iff N_in == 0,
 *   tokens iff N == 0); G <= 0, R <= 0 or G % R != 0; N < 0 or N_in < 0; 128 G, 30 N or 32 N_in >= 2^31; an fp32 or int32
 *   buffer not 4-byte aligned, tokens not 8-byte, tokens_in not 16-byte aligned (the uint8 buffers need no alignment); any
 *   output or workspace overlapping any other buffer (inputs may share memory with each other). */
#define PM_INFILL_SCRATCH(G) (6 * (int64_t)(G) + 2)
int pm_infill_structure(const float* s_in /* [G,4,32] 0/1 */, const uint8_t* s_model /* [G,4,32] */,
                        const uint8_t* region /* [R,4,32] */, int32_t G, int32_t R, float* s_f32 /* [G,4,32] or NULL */,
                        uint8_t* s_u8 /* [G,4,32] or NULL */, int32_t* bar_forced /* [G] */, pm_stream_t stream);
int pm_infill_tokens(const float* s_in /* [G,4,32] 0/1 */, const float* s_out /* [G,4,32] 0/1 */,
                     const uint8_t* region /* [R,4,32] */, int32_t G, int32_t R, const int32_t* tokens_in /* [N_in,16,2] */,
                     int64_t N_in, int32_t* tokens /* [N,15,2] in/out */, int64_t N,
                     const int32_t* bar_forced /* [G] or NULL */, int32_t* scratch /* [PM_INFILL_SCRATCH(G)] */,
                     int32_t* status /* [5] */, pm_stream_t stream);

/* ------------------------------------------------------------------ Note statistics
 * What a batch of pieces held as note events contains, counted on the device, and a subset of its pieces: what "draw several
 * takes of a latent and keep the best by a criterion" needs without a host loop over the notes.  The counts are the small
 * integer reductions behind the objective measures of muspy.metrics (pitch range, pitches and pitch classes used, polyphony,
 * empty beats, groove); the ratios are left to the caller.  Additive, same ABI version.
 *
 * notes [M,3] int32 (time, pitch, duration) and track_ptr [4B+1] int32 are the layout pm_tokens_from_notes reads; every
 * track's range is clamped into [0, M] as there, so nothing outside notes[0:M] and track_ptr[0:4B+1] is read.
 *
 * pm_note_stats: with L = 32 n_bars, a row (t, p, d) of a track is COUNTED iff 0 <= t < L; other rows add to out_of_range and
 * to nothing else.  A counted row is the note the encoder would see: pitch q = clamp(p, 0, 127), duration e = clamp(d, 1, 96),
 * sounding over the steps [t, min(t + e, L)).  Rows need not be sorted and no output depends on their order.  All outputs are
 * int32, one record per (piece, track) in track_ptr order, and every word is written on every call:
 *   track       [4B,12], indexed by PM_NOTE_STAT_*:
 *                 N_NOTES counted rows; N_ONSETS steps with at least one onset; PITCH_MIN lowest q (128 if no note);
 *                 PITCH_MAX highest q (-1 if no note); N_PITCHES distinct q; N_PITCH_CLASSES distinct q mod 12;
 *                 NOTE_STEPS the sum of the clipped lengths min(t + e, L) - t; SOUNDING_STEPS steps at which at least one
 *                 note sounds; POLY_STEPS steps at which at least two sound; MAX_POLYPHONY the largest number of notes
 *                 sounding at one step; MAX_CHORD the largest number of onsets at one step (above 14, pm_tokens_from_notes
 *                 would drop some); OUT_OF_RANGE rows that were not counted.
 *   pitch_class [4B,12]: counted rows per q mod 12.
 *   onsets      [4B,n_bars]: bit s of word b is set iff a counted row has t = 32 b + s (bit 31 is the sign bit: the word is a
 *               bit pattern).
 *   sounding    [4B,n_bars]: the same layout for "at least one note sounds at this step".
 * One launch, a wave per track and the four tracks of a piece per workgroup; the per-step counters (a difference array of the
 * sounding count and the onset count, 2 L int32 per wave) live in LDS, so n_bars <= 64 (64 KB per workgroup).  Integer LDS
 * adds, a wave scan over the steps and wave reductions: no global atomics, no workspace, no host read; two calls on the same
 * input write the same bytes.  12 B are read per row, 96 + 8 n_bars B written per track.  Sums are int32 (NOTE_STEPS wraps
 * beyond 2^31 - 1, more than 22 million notes of a track).
 * PM_E_INVALID (before any launch): a NULL pointer (notes may be NULL when M == 0); B <= 0; n_bars outside [1, 64]; M < 0;
 *   3 M, 4 B n_bars or 48 B >= 2^31; a pointer not 4-byte aligned; an output overlapping an input or another output.
 *
 * pm_notes_select: the pieces index[0..K) of the input, in that order, as notes / track_ptr / totals of their own.
 *   index         [K] int32, K >= 1; entries are to lie in [0, B) and be distinct.  An entry out of range gives an empty piece
 *                 (four equal out_track_ptr entries), and so does an entry that repeats an earlier one: the lowest position
 *                 keeps the piece.  Both are counted, never followed.
 *   out_track_ptr [4K+1]: the scan of the chosen tracks' clamped lengths; out_track_ptr[4K] = M'.
 *   out_notes     [capacity,3]: the chosen rows, unchanged; nothing at or beyond row `capacity` is written and rows from M' on
 *                 are left as they were.  With distinct entries and a track_ptr that does not decrease M' <= M.
 *   out_totals    [2]: M', and the cells: rows whose time differs from the previous row of their track plus one per track that
 *                 is not empty (for tracks sorted by time, the distinct (piece, track, time) triples).
 *   status        [2]: entries out of range, entries that repeat an earlier one.
 *   scratch       PM_SELECT_SCRATCH(B, K) int32: the first position of every input piece, four counts per chosen track.
 * Five launches on the stream (first positions = INT_MAX, their integer minimum over the index, lengths and cells with a wave
 * per chosen track, the scan by one workgroup, the rows), no host read; the minimum is the only atomic and does not depend on
 * arrival order, so two calls on the same input write the same bytes.
 * PM_E_INVALID (before any launch): a NULL pointer (notes may be NULL when M == 0, out_notes when capacity == 0); B <= 0,
 *   K < 1, M < 0 or capacity < 0; 3 M, 3 capacity, 4 B + 1 or the scratch size >= 2^31; a pointer not 4-byte aligned; an output
 *   or the scratch overlapping any other buffer (the inputs may share memory with each other). */
#define PM_NOTE_STAT_N_NOTES 0
#define PM_NOTE_STAT_N_ONSETS 1
#define PM_NOTE_STAT_PITCH_MIN 2
#define PM_NOTE_STAT_PITCH_MAX 3
#define PM_NOTE_STAT_N_PITCHES 4
#define PM_NOTE_STAT_N_PITCH_CLASSES 5
#define PM_NOTE_STAT_NOTE_STEPS 6
#define PM_NOTE_STAT_SOUNDING_STEPS 7
#define PM_NOTE_STAT_POLY_STEPS 8
#define PM_NOTE_STAT_MAX_POLYPHONY 9
#define PM_NOTE_STAT_MAX_CHORD 10
#define PM_NOTE_STAT_OUT_OF_RANGE 11
#define PM_NOTE_STAT_FIELDS 12
#define PM_SELECT_SCRATCH(B, K) ((int64_t)(B) + 16 * (int64_t)(K))
int pm_note_stats(const int32_t* notes /* [M,3] time, pitch, duration */, const int32_t* track_ptr /* [4B+1] */, int32_t B,
                  int32_t n_bars, int64_t M, int32_t* track /* [4B,12] */, int32_t* pitch_class /* [4B,12] */,
                  int32_t* onsets /* [4B,n_bars] */, int32_t* sounding /* [4B,n_bars] */, pm_stream_t stream);
int pm_notes_select(const int32_t* notes /* [M,3] */, const int32_t* track_ptr /* [4B+1] */, int32_t B, int64_t M,
                    const int32_t* index /* [K] */, int32_t K, int32_t* out_notes /* [capacity,3] */, int64_t capacity,
                    int32_t* out_track_ptr /* [4K+1] */, int32_t* out_totals /* [2] */,
                    int32_t* scratch /* [PM_SELECT_SCRATCH(B, K)] */, int32_t* status /* [2] */, pm_stream_t stream);

/* ------------------------------------------------------------------ Note splicing
 * Bar ranges of the pieces of a batch copied into bar ranges of new pieces, on the device: what cuts songs into the model's
 * windows (the reference's sliding window, preprocess.py:165-205: the window by onset time, the two silence filters, the
 * transposition) and what puts windows behind each other in time again.  Additive, same ABI version.
 *
 * notes [M,3] int32 (time, pitch, duration) and track_ptr [4B+1] int32 are the layout pm_tokens_from_notes reads, pieces of
 * src_bars bars; every track's range is clamped into [0, M] as there, so nothing outside notes[0:M] and track_ptr[0:4B+1] is
 * read.  Source tracks need not be sorted by time.
 *
 * pm_notes_splice: K output pieces of out_bars bars.
 *   segments      [S,4] int32, a row (src_piece, src_bar, out_bar, bars); seg_ptr [K+1] int32: output piece j is made of
 *                 segments[seg_ptr[j] : seg_ptr[j+1]], in that order; none gives a silent piece.
 *   rows          track k of output piece j holds, segment by segment, the rows of track k of src_piece whose time t lies in
 *                 [32 src_bar, 32 (src_bar + bars)), in the source's row order, as (t - 32 src_bar + 32 out_bar, pitch,
 *                 duration): a note goes by its onset alone and is never cut (the slice of subsong_content, preprocess.py:171).
 *                 The order is part of the result: it decides the slots pm_tokens_from_notes assigns and which notes past the
 *                 14th of a timestep are dropped.
 *   followed      a segment is followed iff 0 <= src_piece < B, bars >= 1, src_bar >= 0, src_bar + bars <= src_bars,
 *                 out_bar >= the end (out_bar + bars) of the last followed segment of the same output piece, 0 in front of
 *                 the first, and out_bar + bars <= out_bars.  Any other copies nothing and is counted.  seg_ptr is clamped as
 *                 track_ptr is (0 <= lo <= hi <= S); an entry outside [0, S] or below the entry before it is counted.
 *   shift         NULL or [K] int32: the pitches of tracks 1..3 (never the drums) of output piece j become
 *                 clamp(clamp(pitch, 0, 127) + shift[j], 0, 127), preprocess.py:196-205 on the pitch tokens.  NULL leaves every
 *                 pitch as it is.
 *   silence_rule  0 / 1; 1 needs out_bars <= 64.  With act[k][b] = "track k of the output piece has a row in bar b":
 *                 out_bars > 1: keep = 0 if a bar is silent in all four tracks, or if `1 in np.diff(np.where(act == 0)[1])`
 *                 (preprocess.py:182): walking the silent (track, bar) pairs in row-major order, two neighbours whose bars are
 *                 c and c + 1.  That is two consecutive silent bars of one track, and also the last silent bar c of one track
 *                 followed by the first silent bar c + 1 of the next track that has any; out_bars == 1: keep = 0 iff all four
 *                 tracks are silent; else keep = 1.  Pieces with keep = 0 are written like the others; the caller drops them
 *                 (pm_notes_select).  With silence_rule = 0 keep is all ones.
 *   out_notes     [capacity,3]; nothing at or beyond row `capacity` is written, rows from M' on are left as they were.
 *   out_track_ptr [4K+1], the scan of the tracks' rows; out_track_ptr[4K] = M'.
 *   out_totals    [2]: M' (the rows needed, whatever the capacity), and the cells as pm_notes_select counts them: rows whose
 *                 time differs from the previous row of their track plus one per track that is not empty.
 *   keep          [K] 0 / 1.
 *   status        [4]: segments not followed; seg_ptr entries counted; max(M' - capacity, 0); 0.
 *   scratch       PM_SPLICE_SCRATCH(K, S) int32: four counts and the 64-bit mask of bars per output track (nothing is kept
 *                 per segment: the launch that copies walks the segments again with a running base).
 * Three launches on the stream: the counts with a wave per (output piece, track), which scans the source track once per
 * segment; the scan by one workgroup with totals, status and keep; the rows with the same shape, order kept by a ballot and
 * the popcount of the lanes below.  No host read, no atomics: two calls on the same input write the same bytes.  Per segment
 * and track 4 B per source row are read by the count and 4 to 12 B by the copy; 12 B are written per row that goes along.
 * PM_E_INVALID (before any launch): a NULL pointer (notes may be NULL when M == 0, segments when S == 0, out_notes when
 *   capacity == 0, shift always); B <= 0, K < 1, S < 0, M < 0, capacity < 0, src_bars < 1 or out_bars < 1; silence_rule not
 *   0 / 1, or 1 with out_bars > 64; 3 M, 3 capacity, 4 B + 1, 4 S, 32 src_bars, 32 out_bars or the scratch size >= 2^31; a
 *   pointer not 4-byte aligned; an output or the scratch overlapping any other buffer (the inputs may share memory). */
#define PM_SPLICE_SCRATCH(K, S) (24 * (int64_t)(K) + 0 * (int64_t)(S))
int pm_notes_splice(const int32_t* notes /* [M,3] */, const int32_t* track_ptr /* [4B+1] */, int32_t B, int32_t src_bars,
                    int64_t M, const int32_t* segments /* [S,4] */, int32_t S, const int32_t* seg_ptr /* [K+1] */, int32_t K,
                    int32_t out_bars, const int32_t* shift /* [K] or NULL */, int32_t silence_rule,
                    int32_t* out_notes /* [capacity,3] */, int64_t capacity, int32_t* out_track_ptr /* [4K+1] */,
                    int32_t* out_totals /* [2] */, int32_t* keep /* [K] */,
                    int32_t* scratch /* [PM_SPLICE_SCRATCH(K, S)] */, int32_t* status /* [4] */, pm_stream_t stream);

/* ------------------------------------------------------------------ Scores
 * What the decoder thinks of a piece: the log-likelihood of the piece's own tokens and structure under the decoder's logits,
 * per bar and track, with the counts behind the reference's accuracies.  The reference has these terms only as batch means:
 * the cross-entropies with ignore_index = PAD and the BCE with logits of `_losses` (training.py:298-347), the ratios of
 * `_note_accuracy` and its neighbours (training.py:438-468).  Here they stay apart per (bar g = i * n_bars + b of piece i,
 * track k); sums over bars and tracks, ratios, ELBO and importance-weighted bounds are left to the caller.  Additive, same
 * ABI version.
 *
 * pm_score_tokens: nodes are the active cells of s_tensor in cell order, as in pm_node_tracks; a node at or beyond N is
 * ignored.  Row (n, j), j = 0..14, has the logits c_logits[n, j] (131 pitch columns, then 99 duration columns) and the targets
 *   tokens[n, j]      with tok_slots = 15 (the layout pm_sample_tokens writes),
 *   tokens[n, j + 1]  with tok_slots = 16 (pm_tokens_from_notes, BarGraphBatch.tokens: slot 0 is the SOS and is no target).
 * A pitch target is present iff it lies in [0, 130), a duration target iff it lies in [0, 98): PAD (130 / 98, the reference's
 * ignore_index, training.py:101-102) and anything outside the head is absent.  For a head h of a row with a present target t:
 *   logp = (x_t - m) - log sum_c exp(x_c - m), m = max_c x_c over the head's columns, in fp32;
 *   hit  = (t is the head's arg-max, the first index among equal maxima: the rule of pm_content_accuracy).
 *   row_logp    fp32 [N,15,2] (pitch, duration): logp, 0 where the target is absent.
 *   row_verdict uint8 [N,15]: bit 0 pitch hit, bit 1 duration hit, bit 2 pitch target present, bit 3 duration target present.
 *   logp        fp64 [G,4,2]: the sums of row_logp over the rows of the track's nodes.  A node's 15 rows are added in slot
 *               order, the nodes of a track by a fixed tree, all in fp64.
 *   counts      int32 [G,4,6]: nodes, pitch targets, duration targets, pitch hits, duration hits, note hits (pitch AND duration
 *               hit on a row whose pitch target is present: `_note_accuracy`).
 *   scratch     bar_nodes [G] and node_ptr [G+1] as for pm_node_tracks; node_ptr[G] is the number of active cells, which the
 *               caller compares with N.
 * Every word of the four outputs is written on every call, those of bars and tracks without nodes included (zeros); all N
 * rows of row_logp and row_verdict are written whether or not a cell owns the node.  A row whose targets are both absent is
 * not read: 8 B of targets per row, 920 B of logits per row with a target, 9 B written per row; the bar pass reads 135 B per
 * node and writes 160 B per bar.  Four launches on the stream (cells per bar, their scan, the rows, the bars), no host read, no
 * atomics: two calls on the same inputs write the same bytes, and the words of a bar depend on that bar's nodes alone.
 * PM_E_INVALID (before any launch): a NULL pointer (c_logits, tokens, row_logp and row_verdict may be NULL when N == 0);
 *   G <= 0; N < 0; tok_slots other than 15 / 16; 15 N or 128 G >= 2^31; bar_nodes == node_ptr; tokens, row_logp or logp not
 *   8-byte aligned, another fp32 / int32 buffer not 4-byte aligned.
 *
 * pm_score_structure: the Bernoulli log-likelihood of the cells of s_tensor [G,4,32] (a cell is on iff it is non-zero) under
 * s_logits [G,4,32], per (bar, track):
 *   logp   fp64 [G,4] = - sum_t [max(x, 0) - x y + log1p(exp(-|x|))]: the terms in fp32, their 32-term sum in fp64 by a fixed
 *          tree.
 *   counts int32 [G,4,4]: targets on, predictions on, true positives, cells that agree.  The prediction is the one of
 *          pm_structure_metrics, sigmoid(x) >= 0.5.
 * One launch, a bar per half-wave: 1 KB read and 96 B written per bar, no atomics, no workspace.
 * PM_E_INVALID (before the launch): a NULL pointer; G <= 0 or 128 G >= 2^31; logp not 8-byte aligned, another buffer not
 *   4-byte aligned. */
int pm_score_tokens(const float* c_logits /* [N,15,230] */, const int32_t* tokens /* [N,tok_slots,2] */, int32_t tok_slots,
                    const float* s_tensor /* [G,4,32] */, int32_t G, int64_t N, int32_t* bar_nodes /* [G] ws */,
                    int32_t* node_ptr /* [G+1] ws */, float* row_logp /* [N,15,2] */, uint8_t* row_verdict /* [N,15] */,
                    double* logp /* [G,4,2] */, int32_t* counts /* [G,4,6] */, pm_stream_t stream);
int pm_score_structure(const float* s_logits /* [G,4,32] */, const float* s_tensor /* [G,4,32] */, int32_t G,
                       double* logp /* [G,4] */, int32_t* counts /* [G,4,4] */, pm_stream_t stream);

/* ------------------------------------------------------------------ Harmony
 * Pitch rules that follow a chord progression, and the harmony of existing pieces read back as such a rule.  The reference
 * has neither: `generate_music` (generate.py:21-37) decodes every cell on its own and `muspy_from_mtp` (utils.py:126-141)
 * takes what comes out; the rules of pm_sample_chords are per track and fixed for the batch.  Here a chart of pitch-class
 * sets per (bar, step) narrows the draw, and pm_note_chroma counts which pitch classes sound where in a batch of pieces
 * held as notes, so that the harmony of the kept tracks can bind the regenerated ones (an infill) without leaving the
 * device.  Additive, same ABI version.
 *
 * pm_node_cells: node_cell[n] = 128 g + 32 track + step of node n's cell, nodes numbered in cell order as in
 *   pm_node_tracks, whose scratch, tail rule (entries [active, N) are written 0 by the same launch, nothing at or beyond N)
 *   and argument checks it shares; in addition node_cell must be 4-byte aligned and 128 G < 2^31.
 *
 * pm_sample_chords_at: pm_sample_chords with a chart.  The track of node n is (node_cell[n] >> 5) & 3, its bar
 *   g = node_cell[n] >> 7 and its step t = node_cell[n] & 31.
 *   chart      int32 [G,32]: bits 0..11 of chart[g][t] are the pitch classes allowed at step t of bar g; higher bits are
 *              ignored.
 *   track_bits bit k set = the chart binds track k (0 Drums .. 3 Strings).
 *   the pitch rule: for a node of a bound track a pitch p < 128 is a candidate iff pitch_mask[track] allows it AND bit
 *              p % 12 of chart[g][t] is set (and, as ever, it is not used yet and count < max_notes).  For a track that is
 *              not bound the chart is not read.  A set that leaves a node no pitch gives the empty chord, (EOS 129, EOS 97)
 *              in slot 0 and note_count 0, also under min_notes >= 1: the rule pm_sample_chords has for a track whose
 *              candidates run out.
 *   Everything else is pm_sample_chords unchanged: the noise stream and its keys, no pitch twice, the note counts, EOS / PAD.
 *   With track_bits = 0, or with every set 0xfff, the tokens and counts are those of pm_sample_chords bit for bit.
 *   The chart index 32 g + t is clamped into [0, 32 G), so whatever node_cell holds nothing is read outside `chart`.
 *   The chart binds onsets: a note drawn at step t is held for its duration whatever the later sets say.
 *   One wave per node as pm_sample_chords (the same kernel, another instantiation): 4 B of node_cell and, for a bound
 *   track, 4 B of chart are read per node beside the up to 13.8 KB of logits.
 *   PM_E_INVALID (before any launch): what pm_sample_chords refuses; NULL node_cell or chart; G <= 0 or 128 G >= 2^31;
 *   track_bits outside 0..15; c_logits, node_cell, chart, tokens or note_count not 4-byte aligned.
 *
 * pm_note_chroma: the chromagram of the NoteBatch layout (notes [M,3], track_ptr [4B+1], pieces of n_bars bars; see "Note
 *   statistics").  A row counts exactly as in pm_note_stats: 0 <= t < L = 32 n_bars, pitch q = clamp(p, 0, 127), length
 *   e = clamp(d, 1, 96), sounding over the steps [t, min(t + e, L)); track ranges are clamped into [0, M].
 *   seg_steps  1, 2, 4, 8, 16 or 32: the steps of a segment; S = 32 n_bars / seg_steps segments per piece.
 *   chroma     int32 [4B,S,12]: chroma[tr][s][c] = the number of (note, step) pairs of track tr with q % 12 = c whose step
 *              lies in segment s.  Every word is written on every call; the sum over s and c is NOTE_STEPS of pm_note_stats.
 *   One launch, a workgroup per (track, chunk of 16 bars): twelve difference arrays of the chunk's 512 steps in LDS (24 KB),
 *   integer LDS adds, a wave scan and shuffle sums: no global atomics, no workspace, no host read; the result does not
 *   depend on the order of the rows and two calls on the same input write the same bytes.  12 B are read per row and chunk,
 *   48 B written per segment and track.  Sums are int32.
 *   PM_E_INVALID (before any launch): a NULL pointer (notes may be NULL when M == 0); B <= 0; n_bars outside [1, 64];
 *   seg_steps not one of the six; M < 0; 3 M or 48 B S >= 2^31; a pointer not 4-byte aligned; chroma overlapping an input. */
int pm_node_cells(const float* s_tensor /* [G,4,32] 0/1 */, int32_t G, int64_t N, int32_t* bar_nodes /* [G] ws */,
                  int32_t* node_ptr /* [G+1] ws; node_ptr[G] = active cells */, int32_t* node_cell /* [N] */, pm_stream_t stream);
int pm_sample_chords_at(const float* c_logits /* [N,15,230] */, const int32_t* node_cell /* [N] */, int64_t N,
                        const int32_t* chart /* [G,32] */, int32_t G, int32_t track_bits, const PmChordRules* rules,
                        uint32_t seed, int32_t* tokens /* [N,15,2] */, int32_t* note_count /* [N] or NULL */,
                        pm_stream_t stream);
int pm_note_chroma(const int32_t* notes /* [M,3] time, pitch, duration */, const int32_t* track_ptr /* [4B+1] */, int32_t B,
                   int64_t M, int32_t n_bars, int32_t seg_steps, int32_t* chroma /* [4B,S,12] */, pm_stream_t stream);

/* ------------------------------------------------------------------ message aggregation
 * `GCL.message` + PyG `propagate` + torch_scatter mean (model.py:110,123-135):
 *   A[n, r*d:(r+1)*d] = mean_{e: dst=n, type=r} keep_e * relu(x[src_e] * T[dist_e]) / (1-p)
 *   A[n, 6d:7d]       = x[n]                       (root operand of model.py:116)
 * T[dist] = edge_nn.weight[:, dist] + edge_nn.bias  (Linear on a one-hot, model.py:127).
 * keep_e is the counter-based dropout mask pm_dropout_keep(seed, layer, eid, channel). */
int pm_edge_table(const float* nn_weight /* [d,32] */, const float* nn_bias /* [d] */, int32_t d,
                  float* T /* [32,d] */, pm_stream_t stream);
int pm_edge_table_bwd(const float* dT /* [32,d] */, int32_t d, float* d_nn_weight /* += */,
                      float* d_nn_bias /* += */, pm_stream_t stream);
/* compact != 0: the aggregate is [N,4d] = [track block | onset | next | x].  A node only receives track edges of
 * ONE track relation (its own track; data.py:36-49,173-176), so three of the four track blocks of every row are
 * identically zero: the compact form stores the non-zero one (relation PM_PLAN_NODE_TREL[n]) and the GCL GEMM
 * contracts K = 4d instead of 7d (the track block against weight[node_trel], grouped by relation).  Valid only
 * when PM_PLAN_TRK_CNT[4] == 0 (true for every graph built by the reference's rules). */
int pm_segreduce_fwd(const float* x /* [N,d] */, const float* T /* [32,d] */, const int32_t* plan,
                     int32_t N, int32_t E, int32_t G, int32_t d, float dropout_p, uint32_t seed,
                     uint32_t layer_uid, int32_t compact, float* A /* [N,7d] or [N,4d] */, pm_stream_t stream);
/* Same aggregate written PRE-SPLIT for the planes mode of the GEMM: three bf16 planes (value = p1 + p2 + p3 exactly),
 * plane k at planes + k*plane_stride, same [N, 7d | 4d] element layout. */
int pm_segreduce_fwd_planes(const float* x, const float* T, const int32_t* plan, int32_t N, int32_t E, int32_t G,
                            int32_t d, float dropout_p, uint32_t seed, uint32_t layer_uid, int32_t compact,
                            uint16_t* planes, int64_t plane_stride, pm_stream_t stream);
/* GCL.forward (model.py:55-121) of one layer as ONE kernel (gcl.hip): the compact aggregate of 64 rows of a track
 * group is built chunk by chunk in LDS by four producer waves (gather of x rows, GCL.message model.py:123-135,
 * scatter-mean) while four consumer waves contract the previous chunk with the stacked weight [W_t; W_4; W_5; root]
 * (bf16 planes, six products, B fragments straight from `w_frag` = pm_split_planes_frag kind 1 of the layer's [7d, d]
 * weight).  h[n] = A'[n] @ W + bias, bit-identical to pm_segreduce_fwd_planes followed by the grouped planes product;
 * `col_stats` as PmGemmDesc.col_stats; `planes` (optional) receives the A' planes the weight gradient of the backward
 * pass contracts (blocks of row tiles without onset / next receivers are not written when use_classes != 0: the
 * backward never reads them).  d in {128, 256, 512}; the batch must satisfy the compact-GCL premise (track_unique).
 * d = 512 (training.json's width) runs the ring pipeline of wide.hip: eight MFMA waves x 64 of the 512 output columns,
 * the aggregate streamed through the same 2-image LDS ring, the distance table in per-chunk slices. */
int pm_gcl_forward_fused(const float* x /* [N,d] */, const float* T /* [32,d] */, const int32_t* plan, int32_t N,
                         int32_t E, int32_t G, int32_t d, float dropout_p, uint32_t seed, uint32_t layer_uid,
                         const uint16_t* w_frag, const float* bias /* [d] or NULL */, int32_t use_classes,
                         float* h /* [N,d] */, double* col_stats /* [PM_BN_REPL][2][d] += or NULL */,
                         uint16_t* planes /* or NULL */, int64_t plane_stride, pm_stream_t stream);
/* Input gradient of that product, dA'[rows_t] = dh[rows_t] @ [W_t; W_4; W_5; root]^T (the autograd of model.py:104-119),
 * A-stationary (gcl.hip): a workgroup keeps the dh planes of 64 rows of a track group in LDS and walks all 4d output
 * columns; `w_frag_t` = pm_split_planes_frag kind 0 of the layer's [7d, d] weight.  Same result as the grouped planes
 * product with transB (blocks of row tiles without onset / next receivers are not written when use_classes != 0: the
 * segment-reduce backward never reads them).  d in {128, 256, 512}, compact graphs (d = 512: the dh planes stream through
 * the LDS ring of wide.hip once per live 512-column output block instead of staying resident: 192 KB would not fit). */
int pm_gcl_input_grad_fused(const uint16_t* dh_planes /* 3 planes [N,d] */, int64_t plane_stride, const int32_t* plan,
                            int32_t N, int32_t E, int32_t G, int32_t d, const uint16_t* w_frag_t, int32_t use_classes,
                            float* dA /* [N,4d] */, pm_stream_t stream);
/* The same with the BatchNorm backward in front of it (pm_bn_bwd_fused with sums_ready != 0: autograd of model.py:203-206)
 * run in the kernel's prologue instead of as a pass of its own: a workgroup forms dh for its 64 rows from the pre-norm rows
 * `h`, the norm's output gradient `du` and the column sums in `acc3` [PM_BN_REPL][3][d] (pm_segreduce_bwd_norm or
 * pm_bn_bwd_sums), multiplies it as above and WRITES the three dh planes (for pm_gcl_weight_grad_fused afterwards);
 * dgamma / dbeta / dbias_pre (+=, any may be NULL) as pm_bn_bwd_fused.  Same values as the two calls.  d in {128, 256}. */
typedef struct PmBnBwd {
  const float* h;        /* [N,d] input of the norm */
  const float* du;       /* [N,d] gradient of its output */
  const float* mean; const float* var; const float* gamma; const float* beta; /* [d] batch statistics, parameters */
  const double* acc3;    /* [PM_BN_REPL][3][d] column sums of du', du' * xhat, xhat */
  float* dgamma; float* dbeta; float* dbias_pre; /* [d] += or NULL */
  float eps; int32_t relu; /* relu != 0: the norm is followed by a ReLU (du' = du * [BN(h) > 0]) */
  int32_t add_residual;  /* != 0: the self block of dA' leaves as dA'[n, 3d:4d] + du[n] — the residual path of
                            x_i = x_{i-1} + relu(BN(h)), so that pm_segreduce_bwd(_norm) runs with dres = NULL */
  int32_t reserved;
} PmBnBwd;
int pm_gcl_input_grad_bn(const PmBnBwd* norm, uint16_t* dh_planes /* 3 planes [N,d], written */, int64_t plane_stride,
                         const int32_t* plan, int32_t N, int32_t E, int32_t G, int32_t d, const uint16_t* w_frag_t,
                         int32_t use_classes, float* dA /* [N,4d] */, pm_stream_t stream);
/* ---- the fp16 pair operand format ("h2") of the three GCL products at d in {128, 256}
 * An fp32 product on the matrix cores needs its operands split into 16-bit pieces.  The exact three-term bf16 split above
 * costs six MFMA products per fp32 product.  The h2 kernels use Ootomo & Yokota's error-corrected half-precision product
 * instead: v * s = hi + lo with hi, lo fp16 (22 significant bits; s a power of two chosen from the tensor's |max| so that
 * the five-bit exponent of fp16 is not a limit: exact to apply and to undo), and the product runs as the THREE MFMA
 * products hi*hi + hi*lo + lo*hi with fp32 accumulation: element error <= 2^-22 relative plus the dropped lo*lo term of the
 * same size — below the rounding an fp32 dot product of the same length accumulates — at half the matrix-core work, two
 * thirds of the operand bytes (csrc/common.h pm_split2h_pair; parity of the step against the fp64 oracle: tests/).
 * CONDITION: the 2^-22 is relative only for elements with |v s| >= 2^-2, i.e. within 15 binades of the bound the scale is
 * taken from; below, the element error is 2^-25 / s absolute.  One scale serves the whole tensor: a tensor whose bulk lies
 * more than 15 binades below its bound (an outlier channel, a BatchNorm column of tiny variance, a large gradient row — on
 * top of the factor 16 of the dh bound) loses a factor of two of product accuracy per further binade (relative L2 against
 * fp64: 1.2e-6 at 19 binades, 1.9e-5 at 23; tests/test_pair_format_gpu.py holds the products to exactly this model).
 * pm_h2_clamp_events does NOT see it: it counts bounds that were too small, never bounds that were too large.
 * Planes keep the layout and strides of the three-plane format; plane 2 is unused.  d = 512 runs the same format through the
 * ring pipeline of wide.hip (pm_gcl_forward_fused_h2, pm_bn_bwd_fused_h2 + pm_gcl_input_grad_fused_h2, pm_gcl_weight_grad_fused_h2).
 *   absmax_in : device words [PM_ABSMAX_SLOTS] holding float bits whose maximum is max |x| of the kernel's fp32 input (pm_absmax, or a producer's
 *               absmax_out: pm_bn_apply_fused_absmax, PmNormSums.absmax_out); forward: of the layer input x, input gradient: of du
 *   absmax_aux: forward only: the same for the distance table T
 *   scale_out : device float the kernel WRITES: the power of two its activation planes (A' / dh) carry; the weight gradient
 *               undoes both
 *   w_scale   : the power of two the weight planes were built with (pm_split_planes_frag_h2) */
enum { PM_ABSMAX_SLOTS = 64 };   /* a tensor's |max| lives in this many words (the maximum of them counts; one wave reads them with
                                   one load): workgroups add theirs with ONE atomic each, spread over the slots — atomics on one
                                   address serialise at ~150 ns each (4096 of them cost a 10 us launch 37 us more) */
typedef struct PmH2 {
  const uint32_t* absmax_in; const uint32_t* absmax_aux; float* scale_out; float w_scale; int32_t reserved;
} PmH2;
/* out[PM_ABSMAX_SLOTS]: slot = max(slot, float bits of the |max| a workgroup saw) (atomic; the words must start at 0 or at
 * an earlier maximum) */
int pm_absmax(const float* x, int64_t n, uint32_t* out, pm_stream_t stream);
int pm_split_planes_frag_h2(const float* W, int32_t rows, int32_t cols, int32_t kind, int32_t n_mats, int64_t src_stride,
                            int64_t dst_stride, float w_scale, uint16_t* out, pm_stream_t stream);
int pm_gcl_forward_fused_h2(const float* x, const float* T, const int32_t* plan, int32_t N, int32_t E, int32_t G, int32_t d,
                            float dropout_p, uint32_t seed, uint32_t layer_uid, const uint16_t* w_frag, const float* bias,
                            int32_t use_classes, float* h, double* col_stats, uint16_t* planes, int64_t plane_stride,
                            const PmH2* h2, pm_stream_t stream);
int pm_gcl_input_grad_bn_h2(const PmBnBwd* norm, uint16_t* dh_planes, int64_t plane_stride, const int32_t* plan, int32_t N,
                            int32_t E, int32_t G, int32_t d, const uint16_t* w_frag_t, int32_t use_classes, float* dA,
                            const PmH2* h2, pm_stream_t stream);
/* d = 512 (no norm backward inside the input gradient there): the norm's backward pass writing dh planes in the pair format,
 * and the input gradient reading them */
int pm_bn_bwd_fused_h2(const float* x, const float* dy, int32_t O, int32_t C, const float* mean, const float* var, float eps,
                       const float* gamma, const float* beta, int relu, float* dgamma, float* dbeta, float* dbias_pre,
                       double* acc3, uint16_t* dx_planes, int64_t plane_stride, int32_t sums_ready, const PmH2* h2,
                       pm_stream_t stream);
int pm_gcl_input_grad_fused_h2(const uint16_t* dh_planes, int64_t plane_stride, const int32_t* plan, int32_t N, int32_t E,
                               int32_t G, int32_t d, const uint16_t* w_frag_t, int32_t use_classes, float* dA,
                               const float* dh_scale, float w_scale, pm_stream_t stream);
int pm_gcl_weight_grad_fused_h2(const uint16_t* a_planes, int64_t a_plane_stride, const uint16_t* dh_planes,
                                int64_t dh_plane_stride, const int32_t* plan, int32_t N, int32_t E, int32_t G, int32_t d,
                                int32_t use_classes, float* dW, const float* a_scale, const float* dh_scale,
                                pm_stream_t stream);
/* Weight gradient of that product, d[W_t; W_4; W_5; root] += A'[rows_t]^T dh[rows_t] (gcl.hip): 128x128 output tiles,
 * one workgroup per (tile, track group, K slice), operands streamed by loader waves through an LDS ring, K slices added
 * with float atomics; `dW` is the layer's [7d, d] gradient (+=).  Same result as the grouped planes product with transA
 * up to the order of the atomic adds.  d in {128, 256, 512}, compact graphs. */
int pm_gcl_weight_grad_fused(const uint16_t* a_planes /* 3 planes [N,4d] */, int64_t a_plane_stride,
                             const uint16_t* dh_planes /* 3 planes [N,d] */, int64_t dh_plane_stride, const int32_t* plan,
                             int32_t N, int32_t E, int32_t G, int32_t d, int32_t use_classes, float* dW /* [7d,d] += */,
                             pm_stream_t stream);
/* The self block of A' without its round trip through HBM.  Columns [3d, 4d) of the compact aggregate are the root term's
 * operand (model.py:119: the layer's own input row), in the planes: split(x[n]) (pair format: split(x[n] * *scale_out)) —
 * a second copy of a tensor the caller holds until the backward has run.
 *   pm_gcl_forward_fused_sel / _sel_h2: pm_gcl_forward_fused / _h2 with `self_planes`: 0 = those columns of every plane are
 *   NOT written (layout and stride of `planes` unchanged; whatever they held stays); != 0 = the call above.  h, col_stats,
 *   the relation blocks and *scale_out do not depend on it.
 *   pm_gcl_weight_grad_fused_x / _x_h2: pm_gcl_weight_grad_fused / _h2 whose self-block tiles read the rows of `x` [N, d] —
 *   the `x` the forward was given — and split them as the forward did, instead of reading those columns of `a_planes`
 *   (never touched).  The same operand bits, so the same dW: bit-identical in deterministic mode.  N * d * 4 < 2^31. */
int pm_gcl_forward_fused_sel(const float* x, const float* T, const int32_t* plan, int32_t N, int32_t E, int32_t G, int32_t d,
                             float dropout_p, uint32_t seed, uint32_t layer_uid, const uint16_t* w_frag, const float* bias,
                             int32_t use_classes, float* h, double* col_stats, uint16_t* planes, int64_t plane_stride,
                             int32_t self_planes, pm_stream_t stream);
int pm_gcl_forward_fused_sel_h2(const float* x, const float* T, const int32_t* plan, int32_t N, int32_t E, int32_t G, int32_t d,
                                float dropout_p, uint32_t seed, uint32_t layer_uid, const uint16_t* w_frag, const float* bias,
                                int32_t use_classes, float* h, double* col_stats, uint16_t* planes, int64_t plane_stride,
                                const PmH2* h2, int32_t self_planes, pm_stream_t stream);
int pm_gcl_weight_grad_fused_x(const uint16_t* a_planes, int64_t a_plane_stride, const float* x /* [N,d] */,
                               const uint16_t* dh_planes, int64_t dh_plane_stride, const int32_t* plan, int32_t N, int32_t E,
                               int32_t G, int32_t d, int32_t use_classes, float* dW /* [7d,d] += */, pm_stream_t stream);
int pm_gcl_weight_grad_fused_x_h2(const uint16_t* a_planes, int64_t a_plane_stride, const float* x, const uint16_t* dh_planes,
                                  int64_t dh_plane_stride, const int32_t* plan, int32_t N, int32_t E, int32_t G, int32_t d,
                                  int32_t use_classes, float* dW, const float* a_scale, const float* dh_scale,
                                  pm_stream_t stream);
/* The weight products of GCL.forward (model.py:112-119) with the aggregate READ from A' planes (written by
 * pm_segreduce_fwd_planes) instead of built in the kernel: h[n] = A'[n] @ [W_t; W_4; W_5; root] + bias, `col_stats` as
 * above.  The path of dense graphs (BASELINE configs[4]: hundreds of edges per node — the fused kernel's producers keep
 * at most three edges per (node, relation) in flight).  d = 512 (wide.hip). */
int pm_gcl_forward_from_planes(const uint16_t* a_planes /* 3 planes [N,4d] */, int64_t plane_stride, const int32_t* plan,
                               int32_t N, int32_t E, int32_t G, int32_t d, const uint16_t* w_frag,
                               const float* bias /* [d] or NULL */, int32_t use_classes, float* h /* [N,d] */,
                               double* col_stats /* [PM_BN_REPL][2][d] += or NULL */, pm_stream_t stream);
/* ... on planes in the fp16 pair format: two fp16 planes of A' * (*a_scale), written by pm_bar_aggregate_fwd with a PmH2 (whose
 * scale_out is `a_scale`); `w_frag` from pm_split_planes_frag_h2(kind 1) with `w_scale`.  d = 512. */
int pm_gcl_forward_from_planes_h2(const uint16_t* a_planes, int64_t plane_stride, const int32_t* plan, int32_t N, int32_t E,
                                  int32_t G, int32_t d, const uint16_t* w_frag, const float* bias, int32_t use_classes,
                                  float* h, double* col_stats, const float* a_scale, float w_scale, pm_stream_t stream);
/* C[N, Nout] = X[N, K] @ W (+ bias) for a plain linear layer with a short inner dimension, K in {128, 256, 512}, Nout a
 * multiple of K (chord decoder forward model.py:555-559; chord encoder input gradient, autograd of model.py:384-390),
 * A-stationary (linear.hip k_rows_w): the 64 fp32 rows of a tile are split into bf16 planes once and kept in LDS for all
 * output columns.  `w_frag` = pm_split_planes_frag of the weight: kind 0 for W [Nout, K] (y = x W^T), kind 1 for
 * W [K, 32*w_tiles] (y = x W; only the first Nout columns are used).  K = 512: wide.hip (X re-split per 512-column
 * output block, streamed through the LDS ring). */
int pm_rows_times_weight(const float* X, int32_t ldx, int32_t N, int32_t K, const uint16_t* w_frag, int32_t kind,
                         int32_t w_tiles, int32_t Nout, const float* bias /* [Nout] or NULL */, float* C, int32_t ldc,
                         pm_stream_t stream);
/* The same for a long inner dimension and d output columns: C[N, Nout] = X[N, K] @ W, K a multiple of 128, Nout in
 * {128, 256, 512} (chord encoder forward model.py:384-390 without its bias; chord decoder input gradient): producer waves split
 * 64 x 128 fp32 chunks into bf16 planes in an LDS ring, MFMA waves contract them (linear.hip k_rows_wk).  `w_frag`: kind 0
 * for W [Nout, 16*w_pitch] (y = x W[:, :K]^T), kind 1 for W [K, Nout] (y = x W). */
int pm_rows_times_weight_longk(const float* X, int32_t ldx, int32_t N, int32_t K, const uint16_t* w_frag, int32_t kind,
                               int32_t w_pitch, int32_t Nout, float* C, int32_t ldc, pm_stream_t stream);
/* ... and the layer's weight gradient over the same rows: C[M, Nn] += A[:, :M]^T B[:, :Nn] (K rows each; fp32, leading
 * dimensions multiples of 4, M and Nn multiples of 128), colsum_a (optional) [M] += column sums of A — the bias gradient
 * when A is the layer's output gradient.  Six-product bf16 chain as the products above; K slices add with float atomics. */
int pm_rows_tn_weight_grad(const float* A, int32_t lda, int32_t M, const float* B, int32_t ldb, int32_t Nn, int32_t K,
                           float* C /* += */, int32_t ldc, float* colsum_a /* NULL or += */, pm_stream_t stream);
/* pm_segreduce_bwd_norm: as pm_segreduce_bwd, and additionally accumulates the three column sums that the backward of
 * the BatchNorm BELOW needs (dx is that norm's output gradient: x_i = x_{i-1} + relu(BN(h_{i-1})), model.py:203-206)
 * into acc3 [PM_BN_REPL][3][d] (caller-zeroed), so that pm_bn_bwd_fused can run with sums_ready = 1. */
typedef struct PmNormSums {
  const float* h;                  /* [N,d] input of that norm (pre-norm GCL output of the layer below) */
  const float* mean; const float* var; const float* gamma; const float* beta;   /* [d] */
  float eps; int32_t relu;
  double* acc3;
  uint32_t* absmax_out;            /* NULL, or device words [PM_ABSMAX_SLOTS]: atomic max of the float bits of |dx| (PmH2.absmax_in of the layer below) */
} PmNormSums;
int pm_segreduce_bwd_norm(const float* x, const float* T, const float* dA, const float* dres, const int32_t* plan,
                          int32_t N, int32_t E, int32_t G, int32_t d, float dropout_p, uint32_t seed,
                          uint32_t layer_uid, int32_t compact, float* dx, float* dT, const PmNormSums* next_norm,
                          pm_stream_t stream);
int pm_segreduce_bwd(const float* x, const float* T, const float* dA /* [N,7d] or [N,4d] */,
                     const float* dres /* [N,d] or NULL: added to dx (residual path, model.py:206) */,
                     const int32_t* plan, int32_t N, int32_t E, int32_t G, int32_t d, float dropout_p,
                     uint32_t seed, uint32_t layer_uid, int32_t compact, float* dx /* [N,d] */,
                     float* dT /* [32,d] += */, pm_stream_t stream);

/* Bar-resident aggregation (bar.hip): the route of DENSE graphs (BASELINE configs[4]: 127 in-edges per node).  Same maths
 * as pm_segreduce_fwd_planes / pm_segreduce_bwd(_norm) on the compact layout (GCL.message model.py:123-135, propagate /
 * scatter-mean model.py:110, their autograd), but one workgroup owns one bar (edges never leave their bar, data.py:24-121; a bar
 * has at most 4 x 32 nodes — a larger "bar" traps) and a chunk of channels, reads the bar's rows from HBM ONCE into LDS and
 * gathers from there.  Forward: A' [N, 4d] as operand planes — three bf16 planes (`h2` NULL; bit-identical to
 * pm_segreduce_fwd_planes(compact = 1)) or the two fp16 planes of the pair format (`h2`: absmax_in = |max| words of x, absmax_aux
 * = of T, *scale_out receives the power of two the planes carry; w_scale unused); d a multiple of 128.  Backward: dx, dT += and
 * (next_norm non-NULL) the column sums / |dx|max of the norm below, as pm_segreduce_bwd_norm; d a multiple of 64. */
int pm_bar_aggregate_fwd(const float* x, const float* T, const int32_t* plan, int32_t N, int32_t E, int32_t G, int32_t d,
                         float dropout_p, uint32_t seed, uint32_t layer_uid, uint16_t* planes, int64_t plane_stride,
                         const PmH2* h2 /* or NULL */, pm_stream_t stream);
int pm_bar_aggregate_bwd(const float* x, const float* T, const float* dA /* [N,4d] */, const float* dres /* [N,d] or NULL */,
                         const int32_t* plan, int32_t N, int32_t E, int32_t G, int32_t d, float dropout_p, uint32_t seed,
                         uint32_t layer_uid, float* dx /* [N,d] */, float* dT /* [32,d] += */,
                         const PmNormSums* next_norm /* or NULL */, pm_stream_t stream);

/* ------------------------------------------------------------------ dense contraction (fp32 MFMA)
 * C[M,N] (=|+=) op(A)[M,K] * op(B)[K,N] (+ bias[N]) (ReLU), v_mfma_f32_32x32x2_f32.
 * Replaces `addmm`/`mm` of every nn.Linear and of `h @ weight[i]`, `x_r @ root`
 * (model.py:112,116) — with A = [h_0|..|h_5|x] the 7 GEMMs of a GCL are one call.
 * transA: A is stored [K,M]; transB: B is stored [N,K] (nn.Linear weight).
 * rowmap (optional): the gathered dimension (M when !transA, else K) is indirect:
 *   physical row = rowmap[r / rows_per_entry] * rows_per_entry + r % rows_per_entry
 *   and applies to A and C (!transA) or to A and B (transA); `dyn_entries` (device int,
 *   optional) overrides the entry count so no host sync is needed for data-dependent sizes. */
enum { PM_GEMM_RELU = 1, PM_GEMM_ACCUM = 2,
       PM_GEMM_RELU_ADD = 16 /* C = C + relu(op(A) op(B) + bias): the residual tail x + relu(.) of an eval-mode GCL layer
                                whose BatchNorm is folded into the weights (pm_bn_fold_weights); no split-K */,
       PM_GEMM_ZEROED = 8 /* C is known to hold zeros (a pre-cleared arena region): the split-K path of the small head
                             products skips its own clear */,
       PM_GEMM_PARTITION = 4 /* grouped + row lists + device counts: the groups' lists partition at most M (K when
                                transA) rows IN TOTAL; the launch then only enumerates live row panels */ };
/* Tile configurations (host only).  Live ids — fp32 MFMA: 0 = 64x64x16, 2 = 64x64x32 (NN, NT, TN).  Split mode "x6" (fp32
 * operands split exactly into three bf16 terms, six partial products on v_mfma_f32_32x32x16_bf16, fp32 accumulation;
 * error below an fp32 FMA chain; needs 16-byte aligned operands): 4 = 128x128x16, 7 = 128x128x32 (NN, NT),
 * 5 = 128x64x16 (TN).  Pre-split operands (PmGemmDesc.operand_planes): 8 = 64x64x32, 9 = 64x128 with B direct (NN, NT).
 * Ids 1, 3, 6 and 10 are retired: no kernel is built for them and nothing launches them; the numbering is kept because
 * the profiler classes are PM_PROF_GEMM0 + 3 * id + layout.
 * pm_gemm_config: the configuration a PLAIN product of this shape runs on — one group, no row map, fp32 operands that
 *   are 16-byte aligned with contiguous leading dimensions.  It asks the same function as the launch, so for such a
 *   call it is what pm_gemm_f32 launches, a pinned configuration included.  A misaligned operand, a grouped or
 *   row-mapped call can land on an fp32 tile where this reports an x6 one.
 * pm_gemm_force_config (A/B timing): -1 = automatic (default); 0, 2, 4, 5, 7 pin that configuration; any other value
 *   returns PM_E_INVALID and leaves the current choice as it is.  A pinned fp32 id applies to every fp32-operand call.
 *   A pinned x6 id applies to the calls whose operands allow x6 (alignment) and whose layout it has a kernel for
 *   (4, 7: NN / NT; 5: TN); every other call follows the shape rule.  Calls with pre-split operands ignore the pin. */
int pm_gemm_config(int32_t transA, int32_t M, int32_t N, int32_t K);
int pm_gemm_force_config(int32_t cfg);
int pm_gemm_f32(int transA, int transB, int32_t M, int32_t N, int32_t K, const float* A, int32_t lda,
                const float* B, int32_t ldb, float* C, int32_t ldc, const float* bias, int flags,
                int split_k, const int32_t* rowmap, int32_t rows_per_entry, const int32_t* dyn_entries,
                pm_stream_t stream);
/* n_groups independent GEMMs of the same shape bound in ONE launch (blockIdx.y = group): group g uses
 * A + g*a_stride, B + g*b_stride, C + g*c_stride, bias + g*bias_stride (elements), rowmap + g*map_stride and
 * dyn_entries + g*dyn_stride.  With a row map and a device-side count per group this is the per-relation
 * contraction of the compact GCL: h[rows_t] += A'[rows_t, :d] @ weight[t] for the four track relations t. */
int pm_gemm_f32_grouped(int transA, int transB, int32_t M, int32_t N, int32_t K, const float* A, int32_t lda,
                        const float* B, int32_t ldb, float* C, int32_t ldc, const float* bias, int flags,
                        int split_k, const int32_t* rowmap, int32_t rows_per_entry, const int32_t* dyn_entries,
                        int32_t n_groups, int64_t a_group_stride, int64_t b_group_stride, int64_t c_group_stride,
                        int64_t bias_group_stride, int32_t map_group_stride, int32_t dyn_group_stride,
                        pm_stream_t stream);
/* Descriptor form of the grouped GEMM, plus "stacked" operands: when b_split_rows > 0 the STORED rows of B below
 * b_split_rows belong to the group (B + g*b_group_stride) and the rows at and above it are shared by all groups and
 * read from B + b_shared_off + row*ldb.  c_split_rows / c_shared_off do the same for the rows of C when transA (the
 * shared rows are then accumulated atomically by all groups).  This binds the whole compact GCL contraction
 *   h[rows_t] = A'[rows_t, 0:4d] @ [weight[t]; weight[4]; weight[5]; root]        (model.py:112,116)
 * its input gradient and its weight gradient in one launch each. */
/* fp32 -> three bf16 planes with x = p1 + p2 + p3 EXACTLY (8 significand bits each); n % 4 == 0. */
int pm_split_planes(const float* src, int64_t n, uint16_t* planes, int64_t plane_stride /* elements, >= n */,
                    pm_stream_t stream);
typedef struct PmGemmDesc {
  int32_t transA, transB, M, N, K;
  const float* A; int32_t lda;
  const float* B; int32_t ldb;
  float* C; int32_t ldc;
  const float* bias;
  int32_t flags, split_k;
  const int32_t* rowmap; int32_t rows_per_entry;
  const int32_t* dyn_entries;
  int32_t n_groups;
  int64_t a_group_stride, b_group_stride, c_group_stride, bias_group_stride;
  int32_t map_group_stride, dyn_group_stride;
  int32_t b_split_rows; int64_t b_shared_off;
  int32_t c_split_rows; int64_t c_shared_off;
  double* col_stats; /* optional [PM_BN_REPL][2][N] fp64, += : column sums of the stored C values and of their
                        squares (the statistics pass of the BatchNorm that follows, fused into the epilogue; the
                        replica is picked from the row-panel index); !transA, no ACCUM, split_k == 1 */
  int32_t operand_planes; /* != 0: A and B are given PRE-SPLIT as three bf16 planes each (pm_split_planes and the
                        plane outputs of pm_segreduce_fwd / pm_bn_bwd_fused): A / B point at plane 0, the planes are
                        a_plane_stride / b_plane_stride ELEMENTS apart, lda / ldb and the group strides count bf16
                        elements (multiples of 8); the six-product split GEMM then runs without conversion work */
  int64_t a_plane_stride, b_plane_stride;
  const int32_t* class_ptr; /* optional, with row lists: per group 5 boundaries b0..b4 of the list (PM_PLAN_TRK_CNT + 8):
                        rows [b1,b3) have a non-zero second block, rows [b2,b4) a non-zero third block of the
                        [4 x class_block] blocked dimension (K when !transA && !transB, N when transB, M when transA);
                        the all-zero blocks are skipped tile by tile (C tiles that only hold such blocks are left
                        untouched when transB).  Results are unchanged where they are defined. */
  int32_t class_block;
  const void* b_frag;       /* optional, planes mode, !transA: B (a weight matrix, possibly stacked via b_split_rows)
                               additionally as FRAGMENT-MAJOR planes (pm_split_planes_frag: kind 0 when transB, kind 1
                               otherwise, over the whole stored matrix with `ldb` columns).  The kernel then takes its B
                               operands straight from memory into registers (no LDS image of B); used when the shape
                               is aligned with the fragment grid (N % 128 == 0, K % 32 == 0), ignored otherwise. */
  float* a_colsum;          /* optional, transA (weight gradient dW = dy^T x of a linear layer, A = dy stored [K, M]):
                               a_colsum[m] += sum_k A[k, m] — the layer's bias gradient, computed by the same launch
                               (no row map, one group, fp32 operands) */
} PmGemmDesc;
/* Fragment-major bf16 planes of weight matrices W [rows, cols] (fp32; rows, cols multiples of 32) for PmGemmDesc.b_frag:
 * per (32-wide n tile, 16-wide k-step) three contiguous 1 KiB blocks (planes) in MFMA operand order.  kind 0: n = row,
 * k = column (the product uses W transposed: transB); kind 1: k = row, n = column.  out: rows*cols*3 bf16 per matrix. */
int pm_split_planes_frag(const float* W, int32_t rows, int32_t cols, int32_t kind, int32_t n_mats, int64_t src_stride,
                         int64_t dst_stride, uint16_t* out, pm_stream_t stream);
int pm_gemm_f32_desc(const PmGemmDesc* desc, pm_stream_t stream);

/* ------------------------------------------------------------------ batch normalisation
 * nn.BatchNorm1d / BatchNorm2d / PyG BatchNorm (model.py:203,222,228,282,359-375,338,475,638).
 * Tensors are viewed as [O, C, I] (row-major [M,C]: O=M, I=1; NCHW: O=G, I=H*W). */
int pm_bn_stats(const float* x, int32_t O, int32_t C, int32_t I, float* mean /* [C] */,
                float* var /* [C] biased */, float* running_mean /* NULL or [C], updated */,
                float* running_var, float momentum, double* scratch /* [PM_BN_SCRATCH(C)] */, pm_stream_t stream);
int pm_bn_apply(const float* x, int32_t O, int32_t C, int32_t I, const float* mean, const float* var,
                float eps, const float* gamma, const float* beta, const float* residual /* or NULL */,
                int relu, float* y, pm_stream_t stream);
/* dx = BN'(du), du = dy * [relu ? bn(x) > 0 : 1]; dgamma/dbeta accumulate; dbias_pre (optional) += column sums of dx,
 * i.e. the gradient of a bias added right in front of this BatchNorm (GCL.bias, model.py:119 + :203). */
int pm_bn_bwd(const float* x, const float* dy, int32_t O, int32_t C, int32_t I, const float* mean,
              const float* var, float eps, const float* gamma, const float* beta, int relu,
              float* dgamma /* += */, float* dbeta /* += */, float* dbias_pre /* NULL or += */, float* dx,
              double* scratch /* [PM_BN_SCRATCH(C)] */, pm_stream_t stream);
#define PM_BN_SCRATCH(C) (256 * 3 * (C) + 4 * (C))
/* The same two operations in ONE launch each for small batches (row-major [O, C], O <= PM_BN_SMALL_MAX_ROWS: the norms of
 * the heads over B rows, model.py:475,638): statistics (+ running statistics) and apply; backward sums and dx.  No scratch. */
#define PM_BN_SMALL_MAX_ROWS 2048
int pm_bn_small_fwd(const float* x, int32_t O, int32_t C, float eps, const float* gamma, const float* beta,
                    const float* residual /* or NULL */, int relu, float* y, float* mean /* [C] out */,
                    float* var /* [C] biased, out */, float* running_mean /* NULL or [C], updated */, float* running_var,
                    float momentum, pm_stream_t stream);
int pm_bn_small_bwd(const float* x, const float* dy, int32_t O, int32_t C, const float* mean, const float* var, float eps,
                    const float* gamma, const float* beta, int relu, float* dgamma /* += */, float* dbeta /* += */,
                    float* dbias_pre /* NULL or += */, float* dx, pm_stream_t stream);
/* Split forms for synchronised BatchNorm under data parallelism (the reference is single-device, so its
 * BatchNorm statistics span what is here the GLOBAL batch): the column sums of one rank come out as `sums` [3][C] fp64 —
 * statistics mode (dy == NULL): {sum x, sum x^2, 0}; backward mode: {sum du, sum du*xhat, sum xhat} —, the host adds them
 * over the ranks (one all-reduce) and hands the totals back with the global row count O_global * I. */
int pm_bn_partial_sums(const float* x, const float* dy /* or NULL */, int32_t O, int32_t C, int32_t I, const float* mean,
                       const float* var, float eps, const float* gamma, const float* beta, int relu,
                       double* sums /* [3][C] out */, double* scratch /* [PM_BN_SCRATCH(C)] */, pm_stream_t stream);
int pm_bn_stats_from_sums(const double* sums /* [3][C] */, double count, int32_t C, float* mean, float* var,
                          float* running_mean /* or NULL */, float* running_var, float momentum, pm_stream_t stream);
int pm_bn_bwd_from_sums(const float* x, const float* dy, int32_t O, int32_t C, int32_t I, const float* mean,
                        const float* var, float eps, const float* gamma, const float* beta, int relu,
                        const double* sums_local /* [3][C] this rank */, const double* sums_global /* [3][C] all ranks */,
                        double count_global, float* dgamma /* += */, float* dbeta /* += */, float* dbias_pre /* NULL or += */,
                        float* dx, double* scratch /* [2C] */, pm_stream_t stream);

/* ------------------------------------------------------------------ element-wise helpers */
/* Fused forms for row-major [O, C] (I = 1, C % 4 == 0, 16-byte aligned), used by the native step for the GCL norms:
 * `sums` [PM_BN_REPL][2][C] fp64 = column sums of x and x*x, accumulated by the epilogue of the GEMM that produced x
 * (PmGemmDesc.col_stats; PM_BN_REPL replicas spread the atomics, consumers add them up); mean / var / running
 * statistics are written as a side effect (saved for the backward).  pm_bn_bwd_fused accumulates its three column
 * sums into the caller-ZEROED `acc3` [PM_BN_REPL][3][C] fp64 with atomics and needs no finalize launch. */
enum { PM_BN_REPL = 8 };
int pm_bn_apply_fused(const float* x, int32_t O, int32_t C, const double* sums, float eps, const float* gamma,
                      const float* beta, const float* residual /* or NULL */, int relu, float* y,
                      float* mean /* [C] out */, float* var /* [C] out */, float* running_mean /* or NULL */,
                      float* running_var, float momentum, pm_stream_t stream);
/* ... which also leaves max |y| (float bits, atomic max) in absmax_out[PM_ABSMAX_SLOTS]: PmH2.absmax_in of the GCL layer that reads y */
int pm_bn_apply_fused_absmax(const float* x, int32_t O, int32_t C, const double* sums, float eps, const float* gamma,
                             const float* beta, const float* residual, int relu, float* y, float* mean, float* var,
                             float* running_mean, float* running_var, float momentum, uint32_t* absmax_out,
                             pm_stream_t stream);
int pm_bn_bwd_fused(const float* x, const float* dy, int32_t O, int32_t C, const float* mean, const float* var,
                    float eps, const float* gamma, const float* beta, int relu, float* dgamma, float* dbeta,
                    float* dbias_pre /* or NULL */, float* dx /* fp32 output, or NULL with dx_planes */, double* acc3,
                    uint16_t* dx_planes /* or NULL: dx as three bf16 planes (PmGemmDesc.operand_planes) */,
                    int64_t plane_stride /* elements */,
                    int32_t sums_ready /* != 0: acc3 already holds the sums (pm_segreduce_bwd_norm) */,
                    pm_stream_t stream);
/* The column sums of pm_bn_bwd_fused alone: acc3 [PM_BN_REPL][3][C] (caller-zeroed) += sums of du', du' * xhat, xhat. */
int pm_bn_bwd_sums(const float* x, const float* dy, int32_t O, int32_t C, const float* mean, const float* var, float eps,
                   const float* gamma, const float* beta, int relu, double* acc3, pm_stream_t stream);
/* ... which also leaves max |dy| — of the gradient as READ, not of the ReLU-masked du', hence a bound for it — in
 * absmax_dy[PM_ABSMAX_SLOTS] (float bits, atomic max): PmH2.absmax_in of the layer's input gradient */
int pm_bn_bwd_sums_absmax(const float* x, const float* dy, int32_t O, int32_t C, const float* mean, const float* var, float eps,
                          const float* gamma, const float* beta, int relu, double* acc3, uint32_t* absmax_dy,
                          pm_stream_t stream);
/* Eval-mode BatchNorm folded into the linear map in front of it (model.py:203 under `vae.eval()`,
 * generate.py:112): with s = gamma / sqrt(running_var + eps), t = beta - running_mean * s,
 *   W_out[k, n] = W[k, n] * s[n]      (W [rows, cols] row-major, the GCL operand [weight; root] [7d, d])
 *   b_out[n]    = bias[n] * s[n] + t[n]
 * so BN(A @ W + b) = A @ W_out + b_out and the normalisation pass over [N, d] disappears from the forward. */
int pm_bn_fold_weights(const float* W, int32_t rows, int32_t cols, const float* bias, const float* gamma, const float* beta,
                       const float* running_mean, const float* running_var, float eps, float* W_out, float* b_out,
                       pm_stream_t stream);
/* `num_batches_tracked` of all BatchNorm modules after a training forward: counters[i] += inc[i] + [group_cnt[0] > 0] *
 * sel[0][i] + [group_cnt[1] > 0] * sel[1][i] (the embedding norms only count when their node group — drums / non-drums,
 * plan field GROUP_CNT — is non-empty, model.py:362,375). */
int pm_bn_counters_update(int64_t* counters /* [n] */, const int64_t* inc /* [n] */, const int64_t* sel /* [2,n] */,
                          const int32_t* group_cnt /* [2] */, int32_t n, pm_stream_t stream);
int pm_relu_bwd(const float* dy, const float* y, int64_t n, float* dx, pm_stream_t stream);
/* dh = dy * [h > 0], as fp32 (dh, may be NULL) and / or as three bf16 operand planes (planes, may be NULL; plane_stride
 * elements apart): the backward of the GCL layer tail x' = x + relu(h) of a model built with batch_norm = False
 * (model.py:202-206), where pm_bn_bwd_fused stands otherwise.  n % 4 == 0. */
int pm_relu_bwd_planes(const float* dy, const float* h, int64_t n, float* dh, uint16_t* planes, int64_t plane_stride,
                       pm_stream_t stream);
/* y = relu(x) + res (res may be NULL): layer tail of a model built with batch_norm = False (model.py:203-206,219-230). */
int pm_relu_residual_fwd(const float* x, const float* res, int64_t n, float* y, pm_stream_t stream);
/* Element dropout of the cfg.dropout layers (model.py:160,199,244-247,267-270,389-390,473,479,558-559,640) on a
 * row-major [rows, cols] tensor: y = x * keep(seed, site, row, col) / (1 - p) with the counter hash of the message
 * dropout (pm_dropout_hash(seed, site, row, col)); y may alias x; the backward is the same call on the gradient. */
int pm_dropout_rows(const float* x, int64_t rows, int32_t cols, float p, uint32_t seed, uint32_t site, float* y,
                    pm_stream_t stream);
int pm_add(const float* a, const float* b, int64_t n, float* out, pm_stream_t stream);
int pm_colsum_acc(const float* x, int32_t M, int32_t C, int32_t ld, float* out /* [C] += */, pm_stream_t stream);
/* same over an indirect row set (rows = rowmap[r / rpe] * rpe + r % rpe, entry count read on device) */
int pm_colsum_rows_acc(const float* x, int32_t C, int32_t ld, const int32_t* rowmap, int32_t rows_per_entry,
                       const int32_t* dyn_entries, int32_t max_entries, float* out /* [C] += */, pm_stream_t stream);
int pm_reparam_fwd(const float* mu, const float* log_var, const float* eps, int64_t n, float* z, pm_stream_t stream);
int pm_reparam_bwd(const float* dz, const float* log_var, const float* eps, int64_t n, float* dmu /* += */,
                   float* dlog_var /* += */, pm_stream_t stream);

/* ------------------------------------------------------------------ token embedding front
 * ContentEncoder embeddings (model.py:355-377): Linear(131|99 -> d/2) on one-hot tokens is
 * a row lookup, and BatchNorm1d over those rows is a count-weighted statistic of the
 * table, so the stage is: normalise 4 small tables, then gather. */
int pm_embed_tables(const float* w_pitch_drum /* [d/2,131] */, const float* b_pitch_drum,
                    const float* w_pitch_nd, const float* b_pitch_nd, const float* w_dur /* [d/2,99] */,
                    const float* b_dur, const float* bn_drum_g, const float* bn_drum_b,
                    const float* bn_nd_g, const float* bn_nd_b, const float* bn_dur_g, const float* bn_dur_b,
                    float* rm_drum, float* rv_drum, float* rm_nd, float* rv_nd, float* rm_dur, float* rv_dur,
                    const int32_t* tok_hist /* [4][131] */, int32_t d, int training, float eps, float momentum,
                    float* tables /* [4][131][d/2] normalised */, float* stats /* [4][2][d/2] mean,var */,
                    pm_stream_t stream);
int pm_embed_gather(const float* tables, const int32_t* tokens /* [N,16,2] */, const uint8_t* is_drum,
                    int32_t N, int32_t d, int32_t n_slots, float* X /* [N,S,d] */, pm_stream_t stream);
int pm_embed_bwd_scatter(const float* dX /* [N,S,d] */, const int32_t* tokens, const int32_t* plan, int32_t N,
                         int32_t E, int32_t G, int32_t d, int32_t n_slots,
                         float* S /* [4][131][d/2], zeroed by the call */, pm_stream_t stream);
/* PAD tail of the chord encoder when n_slots < 15 (model.py:381-390): forward adds the constant contribution of the
 * all-PAD slots (+ the Linear bias) per node group and applies the ReLU in place; backward adds the tail's exact
 * gradients to chord_encoder.weight[:, S*d:] and to the PAD rows of the token sums. */
int pm_chord_pad_fwd(const float* tables, const float* chord_w /* [d,15d] */, const float* chord_b,
                     const uint8_t* is_drum, int32_t N, int32_t d, int32_t n_slots, float* cvec /* [2][d] scratch */,
                     float* y /* [N,d] in place */, pm_stream_t stream);
int pm_chord_pad_bwd(const float* dy /* [N,d] */, const uint8_t* is_drum, int32_t N, int32_t d, int32_t n_slots,
                     const float* tables, const float* chord_w, float* gsum /* [2][d] scratch */,
                     float* d_chord_w /* += */, float* S /* token sums, += */, pm_stream_t stream);
/* The chord encoder as table algebra (chord.hip; model.py:344-390): its input is a lookup of the four embedding tables, so the
 * Linear(15 d -> d) distributes over it.  Forward: PT [2 groups][S][2 kinds][131][d] = table rows times the slot's weight
 * block (pm_chord_tables_fwd), x0[n] = relu(cvec[group] + the 2 S looked-up rows of PT) (pm_chord_sum_fwd; cvec [2][d] =
 * bias + the all-PAD tail slots, pm_chord_pad_vec).  Backward, dy = gradient of the pre-activation (ReLU mask applied):
 * Gt (layout of PT; the CALLER clears it) += per (group, slot, kind, token) sums of dy rows (pm_chord_sum_bwd: one-hot^T x dy on
 * the matrix cores), from which pm_chord_tables_bwd_w forms d_chord_w[:, :S*d] (+=) and d_chord_b (+= column sums of dy; may be
 * NULL) and pm_chord_tables_bwd_x the token sums S [4][131][d/2] (+= with float atomics: the caller clears S) that
 * pm_embed_tables_bwd takes; the tail slots follow through pm_chord_pad_bwd as before (any order: it only adds).  X [N, S, d]
 * and its gradient are never formed. */
int pm_chord_pad_vec(const float* tables, const float* chord_w, const float* chord_b, int32_t d, int32_t n_slots,
                     float* cvec /* [2][d] */, pm_stream_t stream);
int pm_chord_tables_fwd(const float* tables /* [4][131][d/2] */, const float* chord_w /* [d,15d] */, int32_t d, int32_t n_slots,
                        float* PT, const float* chord_b /* with cvec */, float* cvec /* [2][d] or NULL: as pm_chord_pad_vec, same launch */,
                        pm_stream_t stream);
int pm_chord_sum_fwd(const float* PT, const float* cvec, const int32_t* tokens /* [N,16,2] */, const uint8_t* is_drum, int32_t N,
                     int32_t d, int32_t n_slots, float* x0 /* [N,d] */, pm_stream_t stream);
/* ... which also leaves max x0 (x0 >= 0) in absmax_out[PM_ABSMAX_SLOTS] (float bits, atomic max): PmH2.absmax_in of the first GCL layer */
int pm_chord_sum_fwd_absmax(const float* PT, const float* cvec, const int32_t* tokens, const uint8_t* is_drum, int32_t N,
                            int32_t d, int32_t n_slots, float* x0, uint32_t* absmax_out, pm_stream_t stream);
int pm_chord_sum_bwd(const float* dy /* [N,d] */, const int32_t* tokens, const int32_t* plan, int32_t N, int32_t E, int32_t G,
                     int32_t d /* multiple of 32, <= 512 */, int32_t n_slots, float* Gt, pm_stream_t stream);
int pm_chord_tables_bwd_w(const float* Gt, const float* tables, int32_t d, int32_t n_slots, float* d_chord_w /* += */,
                          float* d_chord_b /* += or NULL */, pm_stream_t stream);
int pm_chord_tables_bwd_x(const float* Gt, const float* chord_w, int32_t d, int32_t n_slots, float* S /* += */, pm_stream_t stream);
int pm_embed_tables_bwd(const float* S, const float* w_pitch_drum, const float* b_pitch_drum,
                        const float* w_pitch_nd, const float* b_pitch_nd, const float* w_dur, const float* b_dur,
                        const float* bn_drum_g, const float* bn_nd_g, const float* bn_dur_g, const float* stats,
                        const int32_t* tok_hist, int32_t d, float eps, float* dw_pitch_drum, float* db_pitch_drum,
                        float* dw_pitch_nd, float* db_pitch_nd, float* dw_dur, float* db_dur, float* dg_drum,
                        float* dbeta_drum, float* dg_nd, float* dbeta_nd, float* dg_dur, float* dbeta_dur,
                        pm_stream_t stream);

/* Synchronised form (data parallel, BatchNorm statistics over the global batch): call once with sums_out [4][2][d/2] fp64
 * (only the local sums {sum_v S[v], sum_v S[v] xhat[v]} per table and channel are written), add them and the token
 * histograms over the ranks, then call again with sums_global / hist_global (sums_out NULL).  All three NULL = the plain
 * form above. */
int pm_embed_tables_bwd_sync(const float* S, const float* w_pitch_drum, const float* b_pitch_drum, const float* w_pitch_nd,
                             const float* b_pitch_nd, const float* w_dur, const float* b_dur, const float* bn_drum_g,
                             const float* bn_nd_g, const float* bn_dur_g, const float* stats, const int32_t* tok_hist,
                             int32_t d, float eps, float* dw_pitch_drum, float* db_pitch_drum, float* dw_pitch_nd,
                             float* db_pitch_nd, float* dw_dur, float* db_dur, float* dg_drum, float* dbeta_drum,
                             float* dg_nd, float* dbeta_nd, float* dg_dur, float* dbeta_dur, double* sums_out,
                             const double* sums_global, const int32_t* hist_global, pm_stream_t stream);

/* ------------------------------------------------------------------ bar pooling / broadcast
 * PyG GlobalAttention over the nodes of each bar (model.py:335-340,408-409) and the
 * bar -> node broadcast `repeat_interleave(out, counts)` (model.py:543-545). */
int pm_gate_fwd(const float* x /* [N,d] */, const float* w /* [d] */, const float* b /* [1] */, int32_t N,
                int32_t d, float* g /* [N] */, pm_stream_t stream);
int pm_attnpool_fwd(const float* x, const float* g, const float* g_mean, const float* g_var, float eps,
                    const float* bn_g, const float* bn_b, const int32_t* plan, int32_t N, int32_t E, int32_t G,
                    int32_t d, float* alpha /* [N] softmax weights */, float* out /* [G,d] */, pm_stream_t stream);
int pm_attnpool_bwd(const float* x, const float* g, const float* g_mean, const float* g_var, float eps,
                    const float* bn_g, const float* alpha, const float* dout /* [G,d] */, const float* gate_w,
                    const int32_t* plan, int32_t N, int32_t E, int32_t G, int32_t d, float* dx /* [N,d] */,
                    float* d_gate_w /* [d] += */, float* d_gate_b /* [1] += */, float* d_bn_g /* [1] += */,
                    float* d_bn_b /* [1] += */, float* scratch /* [3*N + 8] */,
                    const float* x_gate /* NULL, or the gate MLP's own input when it differs from x (dropout in front of
                                           the gate Linear, model.py:160): d_gate_w is then taken against it ... */,
                    float* dx_gate /* ... and the gradient w.r.t. it is written here instead of being added to dx */,
                    pm_stream_t stream);
/* The same in two phases for synchronised BatchNorm of the gate (BatchNorm1d(1) over ALL nodes, model.py:338): phase 1
 * leaves the two local sums {sum dgn, sum dgn * ghat} as fp64 at the head of `scratch` (the host adds them over the
 * ranks), phase 2 takes the global sums and node count. */
int pm_attnpool_bwd_sums(const float* x, const float* g, const float* g_mean, const float* g_var, float eps,
                         const float* alpha, const float* dout, const int32_t* plan, int32_t N, int32_t E, int32_t G,
                         int32_t d, float* scratch /* [3*N + 8] */, pm_stream_t stream);
int pm_attnpool_bwd_from_sums(const float* x, const float* g, const float* g_mean, const float* g_var, float eps,
                              const float* bn_g, const float* alpha, const float* dout, const float* gate_w,
                              const int32_t* plan, int32_t N, int32_t E, int32_t G, int32_t d, float* dx, float* d_gate_w,
                              float* d_gate_b, float* d_bn_g, float* d_bn_b, float* scratch, const float* x_gate,
                              float* dx_gate, const double* sums_global /* [2] */, double count_global,
                              pm_stream_t stream);
int pm_bar_broadcast_fwd(const float* bars /* [G,d] */, const int32_t* plan, int32_t N, int32_t E, int32_t G,
                         int32_t d, float* x /* [N,d] */, pm_stream_t stream);
int pm_bar_broadcast_bwd(const float* dx /* [N,d] */, const int32_t* plan, int32_t N, int32_t E, int32_t G,
                         int32_t d, float* dbars /* [G,d] */, pm_stream_t stream);

/* ------------------------------------------------------------------ structure CNN (4x32 bar grids)
 * CNNEncoder / CNNDecoder convolutions (model.py:219-230,279-285): 3x3, padding 1, NCHW;
 * `up4` fuses nn.Upsample(scale_factor=(1,4)) in front of the convolution (model.py:280-281);
 * pool4 = nn.MaxPool2d((1,4)) (model.py:225). */
int pm_conv3x3_fwd(const float* x, const float* w, const float* b, int32_t G, int32_t Ci, int32_t Co, int32_t H,
                   int32_t W, int up4, float* y, pm_stream_t stream);
int pm_conv3x3_bwd_data(const float* dy, const float* w, int32_t G, int32_t Ci, int32_t Co, int32_t H, int32_t W,
                        int up4, float* dx, pm_stream_t stream);
int pm_conv3x3_bwd_weight(const float* x, const float* dy, int32_t G, int32_t Ci, int32_t Co, int32_t H, int32_t W,
                          int up4, float* dw /* += */, float* db /* += */, pm_stream_t stream);
int pm_maxpool4_fwd(const float* x, int64_t n_out, float* y, pm_stream_t stream);
int pm_maxpool4_bwd(const float* x, const float* dy, int64_t n_out, float* dx, pm_stream_t stream);
/* The conv / norm / pool chains of the model's CNNs in training mode (BatchNorm2d on batch statistics), bar resident: a
 * workgroup keeps its bars in LDS between the launch boundaries that the batch statistics force.  Fixed shapes: s [G,1,4,32],
 * c0 / a0 [G,8,4,32], p0 [G,8,4,8], c1 / a1 [G,16,4,8]; u2 [G,16,4,8], c2 / a2 [G,8,4,32], s_logits [G,1,4,32].  Convolution
 * outputs have the bits of pm_conv3x3_fwd on the same input; statistics are fp64 partial sums per workgroup in `scratch`
 * (`scratch_len` doubles: the grid is sized to it, at most 256 workgroups of 48 / 16 / 1296 doubles), added in a fixed order: no
 * float atomics, the same bits in every run and in both modes.  mean* / var* [C] are written (saved for the backward), rmean* / rvar* (or NULL)
 * updated with `momentum`, as pm_bn_stats does.  c0, a0, c1, a1, c2, a2, da0, dc0: 16-byte aligned.
 * Structure encoder forward, CNNEncoder.conv (model.py:219-230): conv0, BN1, ReLU, MaxPool2d((1,4)), conv4, BN5, ReLU.  3 launches. */
int pm_cnn_enc_fwd(const float* s, const float* w0 /* [8,1,3,3] */, const float* b0, const float* gamma1, const float* beta1,
                   const float* w4 /* [16,8,3,3] */, const float* b4, const float* gamma5, const float* beta5, int32_t G, float eps,
                   float momentum, float* c0, float* a0, float* p0, float* c1, float* a1, float* mean1, float* var1,
                   float* rmean1, float* rvar1, float* mean5, float* var5, float* rmean5, float* rvar5, double* scratch,
                   int64_t scratch_len, pm_stream_t stream);
/* Structure decoder forward, CNNDecoder.conv (model.py:279-285): Upsample((1,4)), conv1, BN2, ReLU, conv4.  2 launches. */
int pm_cnn_dec_fwd(const float* u2, const float* w1 /* [8,16,3,3] */, const float* b1, const float* gamma2, const float* beta2,
                   const float* w4 /* [1,8,3,3] */, const float* b4, int32_t G, float eps, float momentum, float* c2, float* a2,
                   float* s_logits, float* mean2, float* var2, float* rmean2, float* rvar2, double* scratch, int64_t scratch_len,
                   pm_stream_t stream);
/* Backward of pm_cnn_enc_fwd (the autograd of model.py:219-230) from da1 = d(loss)/d(a1): dw*, db*, dgamma*, dbeta* += (each
 * element once, from fp64 sums over the workgroups' partials in `scratch`, conv0's by a one-workgroup launch of its own); da0 [G,8,4,32] is written; dc1 [G,16,4,8] and dc0 [G,8,4,32] are written when not NULL (the input has
 * no gradient).  4 launches. */
int pm_cnn_enc_bwd(const float* s, const float* c0, const float* a0, const float* p0, const float* c1, const float* da1,
                   const float* mean1, const float* var1, const float* gamma1, const float* beta1, const float* mean5,
                   const float* var5, const float* gamma5, const float* beta5, const float* w4, int32_t G, float eps, float* dw0,
                   float* db0, float* dgamma1, float* dbeta1, float* dw4, float* db4, float* dgamma5, float* dbeta5, float* dc1,
                   float* da0, float* dc0, double* scratch, int64_t scratch_len, pm_stream_t stream);

/* ------------------------------------------------------------------ loss (training.py:298-347)
 * Fused softmax cross-entropy of the pitch (131, ignore 130) and duration (99, ignore 98)
 * logits with their gradient, KL divergence, and the structure BCE.  `out` receives
 * {pitch, dur, structure, kld} (float64[4], zeroed by the call). */
/* db_* (optional, all or none, need d_logits): += column sums of d_logits over the drum rows / non-drum rows
 * (pitch block) and all rows (duration block) = gradients of the three un-embedding biases (model.py:561-567). */
int pm_content_ce(const float* c_logits /* [N,15,230] */, const int32_t* tokens /* [N,16,2] */,
                  const int32_t* tok_hist, const uint8_t* is_drum /* [N] or NULL */, int32_t N,
                  int32_t n_slots /* c_logits is [N,S,230] */, float grad_scale,
                  float* d_logits /* or NULL */, float* db_pitch_drum /* [131] or NULL */,
                  float* db_pitch_nd /* [131] */, float* db_dur /* [99] */, double* out, pm_stream_t stream);
/* Same with per-term gradient weights read on the device: dev_scale [2] = {pitch, duration} multiplies d_logits (not the
 * reported loss values).  Data parallel: with dev_scale = n_valid_local * world / n_valid_global the mean of the ranks'
 * gradients is the gradient of the token mean over the GLOBAL batch (training.py:316-323). */
int pm_content_ce_scaled(const float* c_logits, const int32_t* tokens, const int32_t* tok_hist, const uint8_t* is_drum,
                         int32_t N, int32_t n_slots, float grad_scale, const float* dev_scale /* [2] device, or NULL */,
                         float* d_logits, float* db_pitch_drum, float* db_pitch_nd, float* db_dur, double* out,
                         pm_stream_t stream);
/* Fused un-embedding + cross-entropy: the three Linear(d/2 -> 131 | 131 | 99) products of
 * ContentDecoder.forward (model.py:561-567; pitch per drum / non-drum row list of the plan, duration on all rows) and the
 * two CrossEntropyLoss(ignore_index = PAD) terms of `_losses` (training.py:316-323) in one launch: the logits of a
 * 64-row tile stay in the MFMA accumulators, only d_logits [N,S,230] is written (and `logits` when not NULL).
 * H [N,S,d] is the chord decoder's output; out[0] / out[1] receive the pitch / duration loss (zeroed by the call);
 * db_* (all or none) += the bias gradients; dev_scale as in pm_content_ce_scaled.
 * `w_planes`: scratch of pm_unembed_scratch_bytes(d) bytes (bf16 planes of the three weights + accumulator replicas);
 * with it and d/2 in {64, 128, 256} the products run on the bf16 matrix pipe (six products of exact three-way splits,
 * k_unembed_ce_planes); NULL or another width: the fp32-MFMA kernel of round 2. */
int64_t pm_unembed_scratch_bytes(int32_t d);
int pm_unembed_ce(const float* H, const float* w_pitch_drum /* [131,d/2] */, const float* b_pitch_drum,
                  const float* w_pitch_nd, const float* b_pitch_nd, const float* w_dur /* [99,d/2] */, const float* b_dur,
                  const int32_t* tokens, const int32_t* plan, int32_t N, int32_t E, int32_t G, int32_t d, int32_t n_slots,
                  float grad_scale, const float* dev_scale, float* logits /* or NULL */, float* d_logits,
                  float* db_pitch_drum, float* db_pitch_nd, float* db_dur, double* out, uint16_t* w_planes /* or NULL */,
                  pm_stream_t stream);
/* Input gradient of the three un-embeddings (autograd of model.py:561-567) in one launch: dH[rows, :d/2] = d_logits[rows,
 * :131] @ W_pitch (drum / non-drum row lists of the plan), dH[:, d/2:] = d_logits[:, 131:] @ W_dur; d_logits [N,S,230] as
 * pm_unembed_ce leaves it, dH [N,S,d].  Six-product bf16 chain (fp32-exact products); d/2 in {64, 128, 256}.
 * `w_planes`: scratch of pm_unembed_dh_scratch_bytes(d) bytes; a call with prepare != 0 fills it from the weights (needed
 * once per parameter update), a call with prepare == 0 runs the product.  PM_E_UNSUPPORTED when N * n_slots * max(d, 230) * 4
 * >= 2^31 (32-bit byte offsets into d_logits and dH): the caller then runs the three products as GEMMs. */
int64_t pm_unembed_dh_scratch_bytes(int32_t d);
int pm_unembed_dh(const float* d_logits, const float* w_pitch_drum /* [131,d/2] */, const float* w_pitch_nd,
                  const float* w_dur /* [99,d/2] */, const int32_t* plan, int32_t N, int32_t E, int32_t G, int32_t d,
                  int32_t n_slots, float* dH, uint16_t* w_planes, int32_t prepare, pm_stream_t stream);
/* Row lists of the decoder head WITHOUT the rows whose targets are PAD (CrossEntropyLoss(ignore_index), training.py:101-102,316-323:
 * no loss, zero gradient; 30 % of the active-slot rows at the bench's batches): row_lists [3][N*n_slots] — job 0 pitch of the drum
 * nodes' rows, 1 pitch of the other rows, 2 duration of all rows, each ascending; a row stays when its pitch OR its duration target
 * is not PAD —, pad_lists (or NULL) the rows left out in the same layout, row_counts [pm_unembed_row_counts_len(N, n_slots)]
 * (device: [0..2] the lengths of row_lists, [4..6] of pad_lists, the rest scratch), and zeros in the halves of `dH_zero`
 * [N*n_slots, d] (or NULL) that belong to the rows left out.  pm_unembed_ce_rows / pm_unembed_dh_rows are pm_unembed_ce /
 * pm_unembed_dh over such lists (row_counts: three lengths): logits, d_logits and dH of the other rows are not touched (the
 * weight-gradient products take the same lists as row maps). */
int64_t pm_unembed_row_counts_len(int32_t N, int32_t n_slots);
int pm_unembed_row_lists(const int32_t* tokens, const int32_t* plan, int32_t N, int32_t E, int32_t G, int32_t d, int32_t n_slots,
                         int32_t* row_lists, int32_t* pad_lists, int32_t* row_counts, float* dH_zero, pm_stream_t stream);
int pm_unembed_ce_rows(const float* H, const float* w_pitch_drum, const float* b_pitch_drum, const float* w_pitch_nd,
                       const float* b_pitch_nd, const float* w_dur, const float* b_dur, const int32_t* tokens, const int32_t* plan,
                       int32_t N, int32_t E, int32_t G, int32_t d, int32_t n_slots, float grad_scale, const float* dev_scale,
                       float* logits, float* d_logits, float* db_pitch_drum, float* db_pitch_nd, float* db_dur, double* out,
                       uint16_t* w_planes, const int32_t* row_lists, const int32_t* row_counts, pm_stream_t stream);
int pm_unembed_dh_rows(const float* d_logits, const float* w_pitch_drum, const float* w_pitch_nd, const float* w_dur,
                       const int32_t* plan, int32_t N, int32_t E, int32_t G, int32_t d, int32_t n_slots, float* dH,
                       uint16_t* w_planes, const int32_t* row_lists, const int32_t* row_counts, pm_stream_t stream);
/* Weight gradients of the three un-embeddings in ONE launch (autograd of model.py:561-567): dw_pitch_drum / dw_pitch_nd [131, d/2],
 * dw_dur [99, d/2] += d_logits[rows, block]^T H[rows, half] over the plan's drum / non-drum rows and all rows, or over the lists of
 * pm_unembed_row_lists (row_lists / row_counts; NULL: the plan's).  d_logits [N*n_slots, 230], H [N*n_slots, d] (the un-embeddings'
 * input, fp32, 16-byte aligned); d/2 a multiple of 128; bf16 six-product chain, every row read once per 128 columns of d/2, output
 * blocks added with float atomics (not reproducible run to run: deterministic callers use pm_gemm_f32 with the same row maps). */
int pm_unembed_dw(const float* d_logits, const float* H, const int32_t* plan, int32_t N, int32_t E, int32_t G, int32_t d,
                  int32_t n_slots, float* dw_pitch_drum, float* dw_pitch_nd, float* dw_dur, const int32_t* row_lists,
                  const int32_t* row_counts, pm_stream_t stream);
/* Bias gradients (+=) of the three un-embeddings (model.py:561-567) from a given d(loss)/d(logits) [N, S, 230]: column sums
 * of the pitch columns over the drum nodes' / the other nodes' rows and of the duration columns over all rows. */
int pm_unembed_bias_grads(const float* d_logits, const uint8_t* is_drum /* [N] */, int32_t N, int32_t S,
                          float* db_pitch_drums /* [131] */, float* db_pitch_non_drums /* [131] */, float* db_dur /* [99] */,
                          pm_stream_t stream);
int pm_kld(const float* mu, const float* log_var, int32_t B, int32_t d, float beta, float* dmu /* or NULL, += */,
           float* dlog_var, double* out, pm_stream_t stream);
int pm_bce_logits(const float* logits, const float* target, int64_t n, float grad_scale, float* dlogits /* or NULL */,
                  double* out, pm_stream_t stream);

/* ------------------------------------------------------------------ evaluation metrics
 * `_accuracies` (training.py:349-497) as integer counts on the device (the reference takes 9 `.item()` syncs per batch):
 * counts[0..7] = {pitch correct, pitch not-PAD, pitch correct on drum nodes, pitch not-PAD on drum nodes,
 *                 duration correct, duration not-PAD, note (pitch and duration) correct, 0}; slots 1..15 of every node. */
int pm_content_accuracy(const float* c_logits /* [N,15,230] */, const int32_t* tokens /* [N,16,2] */,
                        const uint8_t* is_drum /* [N] */, int32_t N, int64_t* counts /* [8] */, pm_stream_t stream);
/* counts[0..3] = {prediction == target, true positives, predicted positives, target positives},
 * prediction = sigmoid(logit) >= 0.5 (training.py:470-497). */
int pm_structure_metrics(const float* s_logits, const float* s_target, int64_t n, int64_t* counts /* [4] */,
                         pm_stream_t stream);

/* ------------------------------------------------------------------ training accuracies (training.py:174-179)
 * The reference's per-batch `_accuracies` on the training-mode logits, as one int64 counts row [16] per batch:
 *   [0..7] as pm_content_accuracy, [8..11] as pm_structure_metrics, [12] structure cells (G * 128), [13..15] 0.
 * Arg-max over the raw fp32 logits of the pitch (131) and duration (99) blocks, the lowest index on ties (the reference
 * arg-maxes softmax(x): the two differ only where two soft-max values round to the same float).  Two parts: a producer writes
 * one verdict byte per (node, active slot) row r and block — verdict[r] pitch, verdict[N S + r] duration, 1 = arg-max is
 * the target, written for every row whose target is not PAD — and clears counts[0..15]; pm_train_metric_counts then joins the
 * two verdicts of each row (note = pitch and duration) into counts[0..6] and adds the structure counts and [12].
 * pm_unembed_ce_metrics / pm_unembed_ce_rows_metrics: pm_unembed_ce / pm_unembed_ce_rows (loss, d_logits, bias gradients
 * bit-identical) that also produce the verdicts of the rows they cover, then the join (is_drum NULL: no join, the caller
 * issues pm_train_metric_counts).  pm_content_accuracy_slots: the same from materialised logits [N, S, 230]. */
int pm_unembed_ce_metrics(const float* H, const float* w_pitch_drum, const float* b_pitch_drum, const float* w_pitch_nd,
                          const float* b_pitch_nd, const float* w_dur, const float* b_dur, const int32_t* tokens,
                          const int32_t* plan, int32_t N, int32_t E, int32_t G, int32_t d, int32_t n_slots,
                          float grad_scale, const float* dev_scale, float* logits, float* d_logits,
                          float* db_pitch_drum, float* db_pitch_nd, float* db_dur, double* out, uint16_t* w_planes,
                          const uint8_t* is_drum /* [N] or NULL */, uint8_t* verdict /* [2 N n_slots] */,
                          int64_t* counts /* [16] */, pm_stream_t stream);
int pm_unembed_ce_rows_metrics(const float* H, const float* w_pitch_drum, const float* b_pitch_drum, const float* w_pitch_nd,
                               const float* b_pitch_nd, const float* w_dur, const float* b_dur, const int32_t* tokens,
                               const int32_t* plan, int32_t N, int32_t E, int32_t G, int32_t d, int32_t n_slots,
                               float grad_scale, const float* dev_scale, float* logits, float* d_logits,
                               float* db_pitch_drum, float* db_pitch_nd, float* db_dur, double* out, uint16_t* w_planes,
                               const int32_t* row_lists, const int32_t* row_counts, const uint8_t* is_drum /* [N] or NULL */,
                               uint8_t* verdict /* [2 N n_slots] */, int64_t* counts /* [16] */, pm_stream_t stream);
int pm_content_accuracy_slots(const float* c_logits /* [N,S,230] */, const int32_t* tokens /* [N,16,2] */,
                              const uint8_t* is_drum /* [N] or NULL */, int32_t N, int32_t n_slots,
                              uint8_t* verdict /* [2 N S] */, int64_t* counts /* [16] */, pm_stream_t stream);
int pm_train_metric_counts(const int32_t* tokens, const uint8_t* is_drum, const uint8_t* verdict, int32_t N, int32_t n_slots,
                           const float* s_logits /* or NULL */, const float* s_target, int64_t n_cells,
                           int64_t* counts /* [16] */, pm_stream_t stream);

/* ------------------------------------------------------------------ optimiser (train.py:181, training.py:160-166)
 * torch.optim.Adam (no weight decay, no amsgrad) over one flat fp32 buffer. */
int pm_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                 float beta1, float beta2, float eps, int32_t step, float grad_scale, pm_stream_t stream);

/* ------------------------------------------------------------------ guarded optimizer step (training.py:123,160-162)
 * The reference steps Adam through torch.cuda.amp.GradScaler: `scaler.step(optimizer)` skips the update of a step whose
 * gradient holds an inf or NaN — parameters, both moments and Adam's step count stay as they were — and the LR scheduler
 * steps regardless (training.py:168-172).  The entries below give the fused Adam the same skip, decided on the device with
 * no host read; a second cause of a skip is a saturated split of the fp16 pair format (pm_h2_clamp_events) anywhere in the
 * step.  Order of one step on the caller's stream:
 *   pm_overflow_snapshot   before the step's first pair-format launch (the weight planes of the prologue);
 *   pm_overflow_poison     where the gradient travels (a data-parallel exchange, an accumulation over micro-batches): after
 *                          every producer of the gradient has joined, before the exchange (its first element is bucket 0's:
 *                          the all-reduce carries the +inf to every rank, which all decide alike; an accumulation keeps it);
 *   pm_grad_nonfinite_check on the gradient Adam consumes (the reduced one, or the accumulated one), deciding the step;
 *   pm_adam_step_guarded.
 * status: PM_OVF_WORDS uint32 words laid out as below, zeroed by the host once. */
enum {
  PM_OVF_PENDING = 0,    /* causes found since the last guarded step: PM_OVF_NONFINITE_BIT | PM_OVF_SATURATED_BIT */
  PM_OVF_LAST = 1,       /* the causes the last guarded step was skipped for; 0 = it was applied */
  PM_OVF_SNAP = 2,       /* the pair-format saturation counter at the snapshot */
  PM_OVF_N_NONFINITE = 3,/* skipped steps without a saturation on this rank (a non-finite gradient, or another rank's) */
  PM_OVF_N_SATURATED = 4,/* skipped steps with a saturated split on this rank */
  PM_OVF_STEP_SIZE = 5,  /* float bits: lr / (1 - beta1^t) of the last applied step */
  PM_OVF_INV_BC2 = 6,    /* float bits: 1 / sqrt(1 - beta2^t) of the last applied step */
  PM_OVF_TICKET = 7,     /* pm_grad_nonfinite_check's decision word: finished workgroups (bits 0-15), those that saw a
                            non-finite value (bits 16-31); back to 0 when the launch ends */
  PM_OVF_WORDS = 8
};
enum { PM_OVF_NONFINITE_BIT = 1, PM_OVF_SATURATED_BIT = 2 };
/* status[PM_OVF_SNAP] = the saturation counter (one thread).  The counter itself is not changed: pm_h2_clamp_events keeps
 * counting since load / reset.  PM_E_INVALID before pm_h2_clamp_init. */
int pm_overflow_snapshot(uint32_t* status, pm_stream_t stream);
/* If the saturation counter moved since the snapshot: grads[0] = +inf and status[PM_OVF_PENDING] |= PM_OVF_SATURATED_BIT
 * (one thread).  The +inf is what makes an all-reduced (sum: inf + x = inf) or accumulated gradient carry the decision. */
int pm_overflow_poison(float* grads, uint32_t* status, pm_stream_t stream);
/* status[PM_OVF_PENDING] |= PM_OVF_NONFINITE_BIT if any of grads[0..n) is an inf or a NaN — GradScaler's found_inf
 * (training.py:160-162).  Decided on the exponent bits, immune to fast-math flags; one atomic per workgroup.
 * window != 0: a move of the saturation counter since pm_overflow_snapshot sets PM_OVF_SATURATED_BIT too (what
 * pm_overflow_poison records where the gradient travels; a single-rank step without accumulation needs no poison).
 * step == NULL: the flag only.  Otherwise the launch's last workgroup (ticket in status[PM_OVF_TICKET]) DECIDES the optimizer
 * step: it moves status[PM_OVF_PENDING] to status[PM_OVF_LAST] and clears it; no cause: *step += 1 and the bias-correction
 * scalars of the new t into status[PM_OVF_STEP_SIZE / _INV_BC2] (in double, as pm_adam_step forms them on the host); a
 * cause: *skipped += 1 and the cause's counter.  step / skipped: int64 device words. */
int pm_grad_nonfinite_check(const float* grads, int64_t n, uint32_t* status, int64_t* step, int64_t* skipped, float lr,
                            float beta1, float beta2, int32_t window, pm_stream_t stream);
/* pm_adam_step behind the decision of pm_grad_nonfinite_check: every workgroup reads status[PM_OVF_LAST] and the scalars once
 * and stores nothing when a cause is set — what `scaler.step(optimizer)` does on found_inf (training.py:160-162).  Adam's t
 * comes from the device word the decision advanced, never from the host (which cannot know whether the previous step was
 * skipped).  An applied step equals pm_adam_step at the same t bit for bit. */
int pm_adam_step_guarded(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float beta1,
                         float beta2, float eps, float grad_scale, const uint32_t* status, pm_stream_t stream);
/* out[2i], out[2i+1] = the scalars the decision forms for step steps[i] >= 1: lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t)
 * (the same device function; for parity checks against the host formula). */
int pm_adam_bias_scalars(const int64_t* steps, int64_t n, float lr, float beta1, float beta2, float* out,
                         pm_stream_t stream);

/* ------------------------------------------------------------------ gradient clipping by the global norm
 * No line of training.py stands behind these entries: the reference loop does not clip.  They give the fused step what
 * `torch.nn.utils.clip_grad_norm_(vae.parameters(), max_norm)` in front of `optimizer.step()` (training.py:160-166) would
 * give the reference loop, with torch's formula (norm_type 2, error_if_nonfinite=False), decided on the device with no
 * host read, and they record the norm.  Additive, same ABI version.  Order of one optimizer update on the caller's stream,
 * on the gradient Adam consumes (the reduced one, or the accumulated one):
 *   pm_grad_sumsq                  (or pm_grad_nonfinite_check_sumsq in the place of pm_grad_nonfinite_check: one read);
 *   pm_grad_clip_finish;
 *   pm_adam_step_clipped           (status = NULL, or the guarded step's status block).
 * clip: PM_CLIP_WORDS doubles laid out as below; no word needs to be initialised.
 *   sumsq  = sum of partials[0 .. PM_CLIP_PARTIALS), in slot order
 *   norm   = fabs((double)grad_scale) * sqrt(sumsq)         the norm of grad_scale * grads, what Adam consumes
 *   coef   = fmin(1.0, (double)max_norm / (norm + 1e-6))
 *   gscale = (float)((double)grad_scale * coef)             coef == 1.0: gscale == grad_scale exactly
 * A non-finite gradient follows the IEEE arithmetic of these lines and is not special-cased: norm = inf gives coef = 0
 * (inf * 0 = NaN in Adam) or, with max_norm = inf, fmin(1.0, NaN) = 1.0; norm = NaN gives coef = 1.0.  Either way Adam
 * consumes non-finite values, as after torch's clip; the guarded step skips such an update and still records its norm. */
enum {
  PM_CLIP_NORM = 0,        /* norm */
  PM_CLIP_COEF = 1,        /* coef */
  PM_CLIP_GSCALE = 2,      /* gscale, the float's value held in a double */
  PM_CLIP_SUMSQ = 3,       /* sumsq */
  PM_CLIP_PARTIALS_AT = 4, /* the first of the PM_CLIP_PARTIALS per-workgroup sums of squares */
  PM_CLIP_PARTIALS = 256,
  PM_CLIP_WORDS = 260
};
/* partials = per-workgroup sums of (double)g * (double)g over grads[0..n), each in a fixed order, each stored by its
 * workgroup with a plain store; the slots past the launch's grid are zeroed.  Deterministic: the same gradient gives the same
 * bits.  The launch shape of pm_grad_nonfinite_check. */
int pm_grad_sumsq(const float* grads, int64_t n, double* clip, pm_stream_t stream);
/* pm_grad_nonfinite_check and pm_grad_sumsq in one read of the gradient: the same flag and decision as the first, the same
 * partials, bit for bit, as the second. */
int pm_grad_nonfinite_check_sumsq(const float* grads, int64_t n, uint32_t* status, int64_t* step, int64_t* skipped, float lr,
                                  float beta1, float beta2, int32_t window, double* clip, pm_stream_t stream);
/* The formula above from the partials (one workgroup): clip[PM_CLIP_NORM / _COEF / _GSCALE / _SUMSQ], and (norm, coef) into
 * row[0..2) unless row is NULL.  max_norm > 0; +inf measures only. */
int pm_grad_clip_finish(double* clip, float grad_scale, float max_norm, double* row, pm_stream_t stream);
/* pm_adam_step (status == NULL; lr and step as there) or pm_adam_step_guarded (status: the block pm_grad_nonfinite_check*
 * decided in; lr and step ignored) with grad_scale read from clip[PM_CLIP_GSCALE].  The same loops: with coef == 1.0 the
 * step equals pm_adam_step / pm_adam_step_guarded bit for bit; a skipped step stores nothing. */
int pm_adam_step_clipped(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                         float beta1, float beta2, float eps, int32_t step, const double* clip, const uint32_t* status,
                         pm_stream_t stream);

/* ------------------------------------------------------------------ exponential moving average of the parameters
 * No line of training.py stands behind these entries: the reference loop keeps no average.  They give the fused step what
 * `torch.optim.swa_utils.AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(decay))` with `update_parameters` behind
 * every `optimizer.step()` would give the reference loop, inside the Adam launch: the kernel holds the parameter it has just
 * stored, so the average costs 4 bytes more read and 4 more written per parameter instead of a pass of its own, and an
 * update the guarded step skips leaves the average where it was — a decision only the device knows.  Additive, same ABI
 * version.
 *   ema[i] = ema_weight == 1 ? params[i] : ema[i] + ema_weight * (params[i] - ema[i])      ema_weight = 1 - decay
 * with params[i] the fp32 value the step stored (torch's lerp form; a weight of 1 copies, since e + (p - e) is not exactly
 * p in fp32).  fp32 caveat: at decay = 0.9999 an increment below half an ulp of ema[i] is lost until |params[i] - ema[i]|
 * has grown past ulp / (2 ema_weight): the average then lags the exact one; it does not drift away from it. */
/* The superset of pm_adam_step, pm_adam_step_guarded and pm_adam_step_clipped, with the average: params, exp_avg and
 * exp_avg_sq end up bit for bit as those entries leave them.
 *   clip == NULL: the gradient scale is grad_scale; otherwise it is read from clip[PM_CLIP_GSCALE], grad_scale ignored.
 *   status == NULL: step (> 0) and lr come from the host; otherwise the decision and its scalars come from the status
 *   block pm_grad_nonfinite_check* decided in, step and lr ignored, and a skipped step stores nothing — not into ema either.
 * ema: n floats that share no element with the four other buffers.  Its alignment never chooses between the float4 and the
 * scalar kernel (the other four buffers and n do, as in the entries above: the two kernels differ in a last bit of exp_avg,
 * and the average must not move it); the float4 kernel moves an average that is not 16-byte aligned as four floats.
 * PM_E_INVALID: a NULL among the five buffers, such an overlap, a clip that is not 8-byte aligned, n <= 0, or an
 * ema_weight outside (0, 1] (NaN included). */
int pm_adam_step_ema(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n, float lr,
                     float beta1, float beta2, float eps, int32_t step, float grad_scale, float ema_weight,
                     const double* clip, const uint32_t* status, pm_stream_t stream);
/* a[0..n) <-> b[0..n) in place (evaluating, generating and saving from the average without moving the model's parameter
 * buffer): float4 when both are 16-byte aligned and n % 4 == 0, scalar otherwise.  PM_E_INVALID: NULL, n <= 0 or ranges
 * that share an element. */
int pm_buffer_swap(float* a, float* b, int64_t n, pm_stream_t stream);

/* Gradient accumulation over `iters_to_accumulate` micro-batches (training.py:149,158: backward of tot_loss / k, optimizer
 * step every k-th batch): accum = (first ? 0 : accum) + scale * grads, scale = 1 / k. */
int pm_grad_accumulate(const float* grads, float* accum, int64_t n, float scale, int32_t first, pm_stream_t stream);

/* ------------------------------------------------------------------ data-parallel exchange
 * The reference is single-device (train.py:120-122).  Sum-all-reduce of the flat fp32 gradient buffer over RCCL / xGMI
 * for hosts that do not go through torch.distributed: rank 0 makes a 128-byte id (pm_comm_unique_id), the host hands it
 * to every rank, each rank creates its communicator on its current device (pm_comm_init) and then calls pm_allreduce —
 * in place, on `stream`, ordered after the kernels that wrote `buf`.  RCCL is loaded at run time; without it these four
 * return PM_E_UNSUPPORTED and nothing else is affected. */
int pm_comm_unique_id(uint8_t* id128 /* [128] host, out */);
int pm_comm_init(const uint8_t* id128 /* [128] host */, int32_t rank, int32_t world, void** comm /* out */);
int pm_comm_destroy(void* comm);
int pm_allreduce(float* buf, int64_t count, void* comm, pm_stream_t stream);

/* Counter-based dropout mask shared by device code and the oracle (host-callable). */
uint32_t pm_dropout_hash(uint32_t seed, uint32_t layer_uid, uint32_t eid, uint32_t channel);

/* ------------------------------------------------------------------ launch-duration profiler (bench.py roofline)
 * HIP events around GEMM / segment-reduce launches while enabled; pm_prof_end sums the durations per class.  Every event
 * costs ~4 us of GPU idle time, so pm_prof_configure selects WHICH launches are bracketed: the classes of `class_mask`
 * (bit c = class c), every `stride`-th launch of each (default: all classes, every launch).
 * classes 0..32 = GEMM tile configuration (0..10) * 3 + {0 NN, 1 NT, 2 TN}; 33 = segment-reduce forward; 34 = backward.
 * `work` = algorithmic flops (GEMM) or algorithmic HBM bytes (segment-reduce) of the launches. */
enum { PM_PROF_NCLASS_PUBLIC = 35 };
int pm_prof_configure(int64_t class_mask, int32_t stride);
int pm_prof_begin(int32_t max_events);
int pm_prof_end(double* ms /* [35] host */, double* work /* [35] host */, int64_t* count /* [35] host */);

/* ------------------------------------------------------------------ native training step
 * The whole of `PolyphemusTrainer.train`'s inner iteration (training.py:137-166) issued from C++:
 * ~340 kernel launches per step with no interpreter between them.  The model is described by
 * offsets (in floats) into the caller's flat parameter / buffer / gradient arrays, named after the
 * reference's modules; activations live in a caller-provided workspace arena.
 * Four calls so that the data-parallel gradient buckets can be exchanged as soon as they are final:
 *   pm_vae_step_forward  : plan -> encoder -> reparam -> decoder -> losses (+ d loss / d logits)
 *   pm_vae_step_backward_decoder : decoder gradients are final afterwards
 *   pm_vae_step_backward_encoder : encoder head, attention pooling, graph encoder: the gradients of every encoder
 *                                  parameter from `c_encoder.graph_encoder` to the end of the encoder are final
 *   pm_vae_step_backward_encoder_tail : chord encoder, embeddings, structure encoder: all gradients final
 * `state` is a caller-owned HOST blob of pm_vae_step_state_bytes() that carries the saved-activation
 * pointers between the calls.  Training mode only (batch statistics, running stats updated). */
#define PM_MAX_LAYERS 16
typedef struct PmLin { int64_t w, b; } PmLin;              /* offsets into params (and grads)            */
typedef struct PmBn { int64_t w, b, rm, rv; } PmBn;        /* w,b: params; rm,rv: running stats in buffers */
typedef struct PmGcn {
  int64_t nn_w, nn_b;                                       /* shared edge network Linear(32 -> d)          */
  int64_t weight[PM_MAX_LAYERS];                            /* [6,d,d] immediately followed by root [d,d]   */
  int64_t bias[PM_MAX_LAYERS];
  PmBn norm[PM_MAX_LAYERS];
} PmGcn;
typedef struct PmVaeLayout {
  int32_t d, n_bars, n_layers;
  int32_t flags;                                             /* bit 0: the model was built with batch_norm = False: the norms
                                                                of the two GCN stacks and of the two CNNs do not exist
                                                                (model.py:176-188,218-238,278-292; their PmBn entries are unused) */
  /* encoder (model.py:420-483) */
  PmLin enc_conv0; PmBn enc_bn1; PmLin enc_conv4; PmBn enc_bn5; PmLin enc_lin1, enc_lin4, enc_s_bars;
  PmLin enc_pitch_nd, enc_pitch_d, enc_dur; PmBn enc_bn_nd, enc_bn_d, enc_bn_dur; PmLin enc_chord;
  PmGcn enc_gcn; PmLin enc_gate; PmBn enc_gate_bn; PmLin enc_c_bars;
  PmLin enc_merge; PmBn enc_bn_merge; PmLin enc_mu, enc_lv;
  /* decoder (model.py:486-655) */
  PmLin dec_lin; PmBn dec_bn; PmLin dec_s_bars, dec_s_lin1, dec_s_lin4, dec_conv1; PmBn dec_bn2; PmLin dec_conv4;
  PmLin dec_c_bars; PmGcn dec_gcn; PmLin dec_chord, dec_pitch_d, dec_pitch_nd, dec_dur;
  float dropout;                                             /* cfg.dropout: p of the element dropout layers (model.py:160,199,
                                                                244-247,267-270,389-390,473,479,558-559,640); 0 = none */
  int32_t reserved;
} PmVaeLayout;
typedef struct PmBatch {                                    /* device pointers of one collated batch          */
  const int64_t* edge_index; const int32_t* edge_type; const int32_t* edge_dist;
  const int64_t* bars; const int64_t* batch; const uint8_t* is_drum; const int32_t* tokens; const float* s_tensor;
  int32_t N, E, G, B;
  int32_t n_slots;                                          /* active token slots S (1..15), see pm_plan_build */
  int32_t flags;                                            /* bit 0: every node receives edges of at most one track
                                                               relation (host-verified) -> compact GCL, K = 4d;
                                                               bit 1: GCL GEMM operands as pre-split bf16 planes;
                                                               bit 2: also store the content logits (pm_vae_step_outputs)
                                                               — the fused un-embedding + CE otherwise writes d_logits only;
                                                               bit 3: the CALLER computes the loss (pm_vae_step_set_output_grads
                                                               follows): the forward stores the logits and skips its own
                                                               cross-entropy / KLD / BCE and their gradients */
  const float* ce_scale;                                    /* NULL, or device [2]: weights of the pitch / duration CE
                                                               gradients (pm_content_ce_scaled; data-parallel token mean) */
} PmBatch;
/* The step's A/B switches (environment variables PM_GCL_FUSED, PM_GCL_NO_DW, PM_NO_ROWS_W, PM_GCL_NO_CLASSES, PM_FUSED_CE,
 * PM_SIDE_STREAM, PM_SIDE_DELAY_US, PM_DAGG_BN, PM_DAGG_RES, PM_PLAN_SIDE, PM_CHORD_TABLES, PM_H2, PM_BAR_ROUTE, PM_PAD_SKIP, PM_UNEMBED_DW, PM_SENC_FIRST, PM_GCL_OFFSET_LIMIT,
 * PM_GCL_SELF_PLANES, PM_DEBUG: the complete list, csrc/vae_step.hip read_cfg) are read once, when the library is loaded; this re-reads them (host
 * only) so that one process can run one batch through two kernel sets.  Switches of earlier rounds that are no longer read:
 * PM_NO_ROWS_TN, PM_NO_UNEMBED_DH, PM_GCL_NO_BFRAG, PM_DENSE_DEG, PM_LATE_WGRADS, PM_DW_SIDE, PM_FUSED_HEADS. */
int pm_vae_step_reload_switches(void);
int64_t pm_vae_layout_bytes(void);
int64_t pm_vae_step_state_bytes(void);
int64_t pm_vae_step_workspace_bytes(const PmVaeLayout* lay, int32_t N, int32_t E, int32_t G, int32_t B,
                                    int32_t n_slots);
/* Streams: the pm_vae_step_* calls are ordered on `stream` for the caller.  Internally the structure encoder / decoder
 * (model.py:211-299,434-445,500-505) and the parameter-only preparation (weight planes, distance tables) are issued on one
 * further non-blocking stream per device, created by the library on first use, between an event recorded on `stream` and an
 * event `stream` waits for before it reads their results (the structure encoder's backward: forked by
 * pm_vae_step_backward_encoder, joined by pm_vae_step_backward_encoder_tail).  No host synchronisation; capturable.
 * PM_SIDE_STREAM=0 keeps every launch on `stream`.  pm_vae_step_forward builds the plan itself (pm_plan_build). */
int pm_vae_step_forward(const PmVaeLayout* lay, const float* params, float* buffers, float* grads,
                        const PmBatch* batch, int32_t* plan, const float* eps /* [B,d] */, float msg_dropout,
                        uint32_t seed_enc, uint32_t seed_dec, float beta, int structure_loss_on_logits,
                        void* workspace, int64_t workspace_bytes, void* state, double* losses /* [4] dev */,
                        pm_stream_t stream);
/* Introspection of the last forward (host only): info = {compact GCL, bf16-planes GEMM operands, active slots S,
 * fragment-major weight planes built (B-direct GEMM mode), N, E, G, B, then the EFFECTIVE switches of the library —
 * fused un-embedding + cross-entropy (PM_FUSED_CE), second-stream site mask (PM_SIDE_STREAM), deterministic mode,
 * fused GCL kernels (PM_GCL_FUSED), norm backward inside the GCL input gradient (PM_DAGG_BN), chord encoder as table algebra (PM_CHORD_TABLES) —, GCL stacks in the fp16 pair format (bit 0 encoder, 1 decoder),
 * decoder head over the row lists without PAD targets (PM_PAD_SKIP)}.  The parity tests use it to assert that the golden-pinned step IS
 * the measured variant. */
int pm_vae_step_info(const void* state, int32_t* info /* [16] host */);
/* The model outputs of `VAE.forward` (model.py:665-678) as the last forward computed them, copied out of the arena
 * (async on `stream`; any pointer may be NULL): s_logits [G,4,32], c_logits [N,S,230] (active slots only), mu and
 * log_var [B,d].  Valid until the next pm_vae_step_forward on this state. */
int pm_vae_step_outputs(const void* state, float* s_logits, float* c_logits, float* mu, float* log_var,
                        pm_stream_t stream);
/* Introspection for parity tools (host only, no GPU work): where the last forward keeps an activation inside the workspace
 * the caller passed to pm_vae_step_forward — the tensors the backward takes its ReLU decisions from.  stack: 0 = the encoder's
 * GCN, 1 = the decoder's; *byte_offset is relative to the workspace pointer, *numel in floats. */
enum { PM_SAVED_GCN_H = 0,      /* [N,d] pre-norm output of GCL layer `layer` */
       PM_SAVED_GCN_X,          /* [N,d] layer input x_layer (layer = n_layers: the stack's output) */
       PM_SAVED_GCN_XIN,        /* [N,d] the same behind the cfg.dropout layer (= X when the model has no dropout) */
       PM_SAVED_GCN_MEAN, PM_SAVED_GCN_VAR,   /* [d] batch statistics of the layer's norm */
       PM_SAVED_GCN_T,          /* [32,d] distance table of the stack's edge network */
       PM_SAVED_X0,             /* [N,d] chord encoder output (after its ReLU) */
       PM_SAVED_MERGE_PRE, PM_SAVED_MERGE_MEAN, PM_SAVED_MERGE_VAR,   /* encoder.bn_linear_merge: input [B,d], statistics [d] */
       PM_SAVED_DEC_PRE, PM_SAVED_DEC_MEAN, PM_SAVED_DEC_VAR,         /* decoder.batch_norm: input [B,2d], statistics [2d] */
       PM_SAVED_ENC_CNN_LIN1 }; /* [G,d] CNNEncoder.lin[1] output (after its ReLU) */
int pm_vae_step_saved(const void* state, int32_t what, int32_t stack, int32_t layer, int64_t* byte_offset, int64_t* numel);
/* out[r, c] = 1 where the backward of a norm followed by a ReLU lets the gradient through: (x - mean) * rsqrt(var + eps) *
 * gamma + beta > 0, evaluated by the expression the backward kernels use (csrc/common.h pm_bn_bwd_elem). */
int pm_bn_relu_decisions(const float* x /* [rows,C] */, const float* mean, const float* var, const float* gamma, const float* beta,
                         float eps, int64_t rows, int32_t C, uint8_t* out /* [rows,C] */, pm_stream_t stream);
/* The drop-in module's path — `model(graph)` called by the unchanged training.py:137-166, which computes `_losses` itself
 * and calls `backward()`: between pm_vae_step_forward (PmBatch.flags bit 2: keep the logits) / pm_vae_step_outputs and the
 * four backward calls the caller hands in the gradients of the four outputs (any may be NULL = zero; d_c_logits covers the
 * step's S slots, [N, S, 230]; d_s_logits != NULL switches the structure decoder's backward on).  They replace the
 * gradients of the step's own loss kernels. */
/* Training accuracies of the step (host only, no GPU work): every following pm_vae_step_forward on `state` (until the next call)
 * writes the counts row of its batch into `counts` (device int64 [16], the layout of pm_train_metric_counts; NULL = off, the
 * default).  The fused head's metrics instantiation writes the verdicts (the unfused head: pm_content_accuracy_slots), one
 * count launch behind the structure loss joins them; no host synchronisation.  The verdicts take 2 N S bytes at the end of the
 * workspace (pm_vae_step_workspace_bytes includes them).  A forward with PmBatch.flags bit 3 (the caller's loss) counts nothing. */
int pm_vae_step_set_metrics(void* state, int64_t* counts);
int pm_vae_step_set_output_grads(void* state, const float* d_s_logits /* [G,4,32] */, const float* d_c_logits /* [N,S,230] */,
                                 const float* d_mu /* [B,d] */, const float* d_log_var /* [B,d] */, pm_stream_t stream);
/* The outputs of the last forward and the buffers their gradients are read from, as byte offsets into the workspace given to
 * pm_vae_step_forward (host only): [0..3] = s_logits [G,4,32], c_logits [N,S,230], mu [B,d], log_var [B,d]; [4..7] = the
 * gradient buffers in the same order.  A caller that writes a gradient into its buffer passes that pointer to
 * pm_vae_step_set_output_grads (no copy); any other d_c_logits pointer is used where it lies (no copy either: it must stay
 * alive, 16-byte aligned, until the four backward calls have run). */
int pm_vae_step_output_views(const void* state, int64_t* byte_offset /* [8] */, int64_t* numel /* [8] */);
/* ORDERING CONTRACT of the decoder's gradients: pm_vae_step_backward_decoder returns with the weight gradients of the decoder's
 * head (un-embeddings, chord decoder, the two head products) still running on the library's second stream, NOT yet joined to
 * `stream`.  They are final for the caller only behind pm_vae_step_join_decoder_grads, pm_vae_step_backward_encoder_heads or
 * pm_vae_step_backward_encoder (each makes `stream` wait for them).  A host that reads, synchronises on, or all-reduces the
 * decoder's gradients directly after this call MUST call pm_vae_step_join_decoder_grads first. */
int pm_vae_step_backward_decoder(void* state, pm_stream_t stream);
/* Data parallel: the weight gradients of the decoder's head run on the library's second stream beside the head chain and
 * are joined inside pm_vae_step_backward_encoder; a caller that hands the decoder's gradient bucket to an all-reduce
 * between the two calls makes `stream` wait for them with this call first (no-op when nothing is open). */
int pm_vae_step_join_decoder_grads(void* state, pm_stream_t stream);
/* The head chain of the encoder backward as a call of its own (optional: pm_vae_step_backward_encoder runs it when it has
 * not been called).  It returns with `stream` waiting for the decoder's weight gradients WITHOUT a stall (they have ~0.5 ms
 * of head chain beside them): a data-parallel caller launches the decoder's gradient bucket behind it, in front of the
 * encoder's GCN stack. */
int pm_vae_step_backward_encoder_heads(void* state, pm_stream_t stream);
int pm_vae_step_backward_encoder(void* state, pm_stream_t stream);
int pm_vae_step_backward_encoder_tail(void* state, pm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* POLYPHEMUS_HIP_H */
