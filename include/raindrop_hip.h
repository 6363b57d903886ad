/*
 * raindrop_hip.h -- C-ABI of libraindrop_hip.so, the MI355X (gfx950) implementation of the
 * Raindrop hot path: Raindrop_v2.forward and its backward.
 *
 * The reference (/root/reference, pure Python on PyTorch + PyTorch-Geometric) has NO native
 * interface for this path; its "FFI" is the set of torch / PyG / torch_scatter op call sites in
 *   code/models_rd.py:278-387      (Raindrop_v2.forward)
 *   code/Ob_propagation.py:94-228  (Observation_progation.forward / message / aggregate)
 *   code/transformer_conv.py:139-207
 * Each entry point below names the call sites it replaces.  Host binding: ctypes
 * (raindrop_amd/_lib.py); see INTEGRATION.md for the stub a reference maintainer would add.
 *
 * Conventions (all entry points):
 *   - plain pointers and sizes only; every tensor pointer is DEVICE memory owned by the caller
 *     (the library never allocates, frees or retains tensor memory); fp32 unless stated;
 *     "int64" tensors are torch.int64; masks are 1 byte per element (torch.bool);
 *   - work is enqueued asynchronously on `stream` (a hipStream_t passed as void*); no host
 *     synchronisation, no internal streams, safe to capture into a hipGraph;
 *   - scratch memory comes from the caller: query rd_*_workspace_bytes(), pass a buffer that
 *     stays alive until the stream has run the call;
 *   - return 0 on success, RD_EINVAL / RD_EUNSUPPORTED (negative) for argument errors detected
 *     before any launch, or a positive hipError_t from the launch; rd_last_error() returns a
 *     thread-local message for the last non-zero return;
 *   - re-entrant; results are deterministic (no floating-point atomics).  The library keeps no per-call state.  Two
 *     settings exist outside the call arguments: the arithmetic mode (rd_set_precision, process-wide, meant to be chosen
 *     once at start-up) and the dropout seed cell (rd_set_seed_cell, per host thread, read at enqueue time).
 */
#ifndef RAINDROP_HIP_H
#define RAINDROP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RD_OK 0
#define RD_EINVAL (-1)
#define RD_EUNSUPPORTED (-2)

#define RD_ABI_VERSION 1

/* Arithmetic of the dense contractions (inputs, outputs and accumulation are always fp32):
 *   RD_PREC_FP32   v_mfma_f32_16x16x4_f32, bitwise an fp32 fmaf chain (157 TF/s peak)
 *   RD_PREC_BF16X3 each fp32 operand split into bf16 hi+lo, products hi*hi + hi*lo + lo*hi on
 *                  v_mfma_f32_16x16x32_bf16 with fp32 accumulate: ~2^-16 relative per product
 *                  (fp32-class after accumulation; logits agree with the fp32 path to ~1e-6),
 *                  5.3x the MFMA throughput.  Default; env RD_PRECISION=fp32 selects the other. */
#define RD_PREC_FP32 0
#define RD_PREC_BF16X3 1
/*   RD_PREC_BF16   operands rounded to bf16 (hi part only), ONE product per MFMA step, fp32 accumulate: the arithmetic of
 *                  BASELINE.json's "P12 ... bf16" configuration (~2^-9 per product; logits within 3e-2 of the fp32
 *                  reference).  Dense layers of the encoder / head / generic message passing only; the fused
 *                  K1 path, attention, softmax, LayerNorm stay as in the other modes.  env RD_PRECISION=bf16. */
#define RD_PREC_BF16 2

/* Problem shape shared by the model-level entry points.
 * K = T*d_ob (channels per sensor node), Dm = F*d_ob, D = Dm + d_pe (transformer width). */
typedef struct rd_shape {
  int32_t B;         /* samples in this batch (columns of src)                                  */
  int32_t T;         /* time steps == max_len (code/models_rd.py:243: Linear(max_len*d_ob, .))  */
  int32_t F;         /* sensors, d_inp                                                          */
  int32_t d_ob;      /* observation-embedding width per sensor (code/Raindrop.py:126 -> 4)      */
  int32_t d_pe;      /* positional-encoding width (code/models_rd.py:216 -> 16)                 */
  int32_t nhead;     /* attention heads (code/Raindrop.py:130 -> 2)                             */
  int32_t nhid;      /* FFN width (code/Raindrop.py:128 -> 2*F*d_ob)                            */
  int32_t d_static;  /* static feature width, 0 when the model has no static branch            */
  int32_t n_classes;
  int32_t max_len;   /* PE timescale base (== T for the shipped configs)                        */
} rd_shape;

/* ---- library identity -------------------------------------------------------------------- */
int rd_version(void);             /* RD_ABI_VERSION                                           */
const char* rd_arch(void);        /* "gfx950"                                                  */
const char* rd_last_error(void);  /* thread-local; "" if none                                  */
int rd_set_precision(int32_t mode); /* process-wide; RD_PREC_*                                 */
int rd_get_precision(void);
/* Dropout seeds are passed by value, which a captured hipGraph freezes.  If a device cell is
 * registered, every dropout kernel adds its content to the seed it was launched with; bumping the
 * cell (a 1-thread kernel, itself capturable) gives each graph replay fresh masks while forward and
 * backward of one step still agree.  Pass NULL to unregister.  The registration is per HOST THREAD and is consumed
 * when a call is ENQUEUED (the pointer is passed to the kernels as an argument): register it around the enqueue or the
 * stream capture of a step and unregister afterwards -- a captured graph keeps using the cell it was captured with, and
 * calls made while no cell is registered are unaffected by it.  The cell must outlive every launch that received it. */
int rd_set_seed_cell(const uint64_t* device_cell);
int rd_seed_cell_advance(uint64_t* device_cell, uint64_t delta, void* stream);

/* Side branch for trailing launches.  rd_set_side_stream registers (per host thread, consumed when a call is enqueued; NULL
 * clears) a second stream: launches that only produce parameter gradients nothing later in the backward pass reads -- the slice
 * reduces of rd_encoder_layer_bwd's weight-gradient stream, rd_head_train's weight-gradient tiles and loss mean -- are then
 * ordered behind the caller's stream and enqueued THERE, beside whatever the caller enqueues next.  The caller owns the join:
 * rd_side_join(stream) makes `stream` wait for the side branch (call it before reading those gradients / the loss on `stream`,
 * and before the end of a stream capture that forked).  With no side stream registered nothing changes.  Results are identical
 * either way (the same kernels on the same data; only their overlap changes). */
int rd_set_side_stream(void* stream);
int rd_side_join(void* stream);

/* Deferred trailing launches (round 4; what replaced the side branch as the default of raindrop_amd.step.TrainStep).  With
 * rd_set_defer_trailing(1) (per host thread, consumed at enqueue) the same launches are not enqueued at all but PARKED -- one at a
 * time -- and the next rd_encoder_layer_bwd that runs its fused backward chain appends them to that launch as extra workgroups, which
 * run on the CUs the chain leaves idle.  A parked launch nobody picks up runs stand-alone when the next one is parked or when
 * rd_flush_trailing(stream) is called: call it before reading those gradients / the loss, and before the end of a stream capture.
 * Results are identical in every mode (same arithmetic on the same data).
 * Two rules for a C-ABI caller: (1) a parked slice reduce of layer i -- including the LayerNorm dgamma / dbeta column sums over the
 * layer's partial matrices -- runs INSIDE layer i-1's backward launch, beside workgroups that rewrite the partials and row tiles of
 * the workspace THEY were given: while the mode is on, every layer needs its OWN rd_encoder_layer workspace until
 * rd_flush_trailing (raindrop_amd.step.TrainStep: `enc_wss`); sharing one workspace across layers is only legal with the mode off.
 * (2) The slot holds raw device pointers.  rd_set_defer_trailing(0) and rd_set_side_stream(NULL) DISCARD whatever is still parked
 * (so does rd_drop_trailing): leave the mode through them on every error path, flush before leaving it on the normal one. */
int rd_set_defer_trailing(int32_t on);
int rd_flush_trailing(void* stream);
int rd_drop_trailing(void);

/* ---- token plan: the padding mask as a layout --------------------------------------------------------------------------
 * code/models_rd.py:298-299 builds mask[b,t] = (t >= lengths[b]) and uses it twice: as src_key_padding_mask of the encoder
 * (:358) and in the masked mean (:366-367,379).  Between them the two uses remove every padded step from the logits AND from
 * every gradient (its rows of the encoder's activation gradients are exactly zero).  rd_token_plan turns `lengths` into a
 * layout: samples ordered by descending length (ties by index), sample b's live steps t < min(lengths[b], T) at rows
 * off[rank[b]] + t of every [tokens, *] tensor.  While a plan is registered (rd_set_token_plan: per host thread, consumed when a
 * call is ENQUEUED, like the seed cell), rd_sensor_stage_fwd, rd_encoder_layer_fwd/bwd, rd_head_train, rd_masked_mean_fwd and rd_msgpass_bwd read and
 * write ONLY those rows -- buffers keep their padded sizes, the first plan[0] rows are used -- and skip the arithmetic whose
 * operand is an exactly-zero padded step.  Logits, loss and all parameter gradients are the same function of the inputs as
 * without a plan (up to the order of the fp32 sums over tokens); z / x / dx at padded steps, which nothing reads, are not
 * produced.  Supported where the step runs on plan-aware kernels: a bf16 arithmetic mode, d_ob = 4, the fused row-local encoder
 * chains (ceil(D / 32) == 5, ceil(nhid / 32) == 9: P19 and P12), head_dim <= 96, the fused head -- at any T (T <= 64: in_proj + attention
 * as one launch per direction, rd_attnfuse.hip; beyond: the multi-tile attention kernels on plan rows) and with either message-passing
 * form (fused LDS-resident, or the panel products whose last scatter follows the plan; rd_pe_mask writes the PE rows the same way).
 * The row-block path also needs ceil(3 D / 32) == 15 (in_proj's input gradient), so the encoder widths a plan runs at are D = 152 .. 160:
 * D = 136 / 144, which the fused attention launch alone would take, are refused.  A length of 0 is legal: such a sample owns no row and
 * contributes to no gradient (tests/test_plan_layer_gpu.py holds both).
 * Other shapes / modes are refused while a plan is registered -- rd_encoder_layer_fwd / _bwd / _fwd_infer with RD_EINVAL ("token plan:
 * ...") before any launch, kernels further down with RD_EUNSUPPORTED (raindrop_amd.step.plan_supported is the host-side test).
 * plan_out: rd_token_plan_bytes(s) bytes of int32 (layout: raindrop_amd/csrc/rd_plan.h; [0] = live rows, [1] = their 32-row chunks,
 * [5] = chunks of the per-sample chunk space the fused attention exports its weight-gradient row tiles in; per-rank off / len,
 * per-sample rank / first row / length).  If seed_cell is not NULL the launch also adds `delta` to it (rd_seed_cell_advance folded
 * in: one launch fewer per step). */
size_t rd_token_plan_bytes(const rd_shape* s);
int rd_token_plan(const rd_shape* s, const int64_t* lengths, int32_t* plan_out, uint64_t* seed_cell, uint64_t delta,
                  void* stream);
int rd_set_token_plan(const int32_t* device_plan);

/* ---- a5/a6: integer work (bit-exact contracts) -------------------------------------------- */

/* code/models_rd.py:307-311: adj = global_structure; adj[diag] = 1; edge_index =
 * nonzero(adj).T (row-major; row 0 = source j, row 1 = target i); edge_weights = adj[r, c].
 * adj_out [F,F] receives the diagonal-patched adjacency (the reference patches its input in
 * place); edge_index is int64 [2, F*F] capacity with row stride F*F, edge_weights [F*F],
 * n_edges int32[1].  Entries beyond n_edges are left untouched. */
int rd_graph_build(int32_t F, const float* global_structure, float* adj_out, int64_t* edge_index,
                   float* edge_weights, int32_t* n_edges, void* stream);

/* code/models_rd.py:298-299: mask[b,t] = (t >= lengths[b]) as bytes [B,T];
 * code/models_rd.py:28-38,292,354: pe[t,b,:] = [sin(times/ts), cos(times/ts)] written into
 * columns [F*d_ob, F*d_ob + d_pe) of the concat buffer z [T,B,D]; timescales[d_pe/2] are
 * computed by the host in float64 and passed as fp32, exactly as the reference casts them. */
int rd_pe_mask(const rd_shape* s, const float* times, const int64_t* lengths,
               const float* timescales, float* z, uint8_t* mask, void* stream);

/* ---- a7-a13: inter-sensor message passing (kernel K1) ------------------------------------- */

/* PyG `softmax(edge_weights, index=target)` + per-target coefficient sum on the dense sensor
 * graph (code/Ob_propagation.py:187,195 via models_rd.py:307-311): for the patched adjacency
 * adj [F,F] (edge j->i exists iff adj[j,i] != 0) writes gamma[j,i] = softmax over sources j of
 * adj[:,i] (0 where no edge) and ssum[i] = sum_j gamma[j,i].  One wavefront per target node,
 * wave-shuffle reductions; F <= 1024. */
int rd_edge_softmax(int32_t F, const float* adj, float* gamma, float* ssum, void* stream);

/* The same softmax over an explicit edge list (duplicate edges allowed): edge_index int64 with
 * rows [source; target] `row_stride` elements apart, normalised by row `norm_row`
 * (1 = target: code/Ob_propagation.py:195, code/transformer_conv.py:201; 0 = source: the
 * use_beta branch, code/Ob_propagation.py:184).  gamma_e [E], ssum [N]. */
int rd_edge_softmax_list(int32_t N, int32_t E, const int64_t* edge_index, int64_t row_stride,
                         int32_t norm_row, const float* edge_weights, float* gamma_e, float* ssum,
                         void* stream);
/* The same followed by F.dropout(gamma, p) (code/Ob_propagation.py:196, code/transformer_conv.py:203; training mode of an operator
 * constructed with dropout > 0 -- the shipped model uses 0): gamma_e[e] is 0 or gamma / (1 - p), ssum the sum of THOSE; the mask is
 * a function of (seed + the registered seed cell, edge index). */
int rd_edge_softmax_list_dropout(int32_t N, int32_t E, const int64_t* edge_index, int64_t row_stride, int32_t norm_row,
                                 const float* edge_weights, float p_drop, uint64_t seed, float* gamma_e, float* ssum, void* stream);

/* Source-valued aggregate of TransformerConv (code/transformer_conv.py:158,168-175,205-206) on a
 * dense coefficient matrix: out[i,c] = sum_j gamma[j,i] V[j,c] (+ skip[i,c] if skip != NULL);
 * backward w.r.t. V: dV[j,c] = sum_i gamma[j,i] dout[i,c]. */
int rd_aggregate_fwd(int32_t N, int32_t C, const float* gamma, const float* V, const float* skip,
                     float* out, void* stream);
int rd_aggregate_bwd(int32_t N, int32_t C, const float* gamma, const float* dout, float* dV,
                     void* stream);

/* The GENERAL message / aggregate of the reference's TransformerConv (code/transformer_conv.py:186-207; round 6): H heads of C
 * channels, scores from the projections instead of given edge weights --
 *   alpha[e,h] = softmax over the edges into tgt(e) of <q[tgt(e),h], k[src(e),h] + edge_feat[e,h]> / sqrt(C)   (edge_feat =
 *   lin_edge(edge_attr) [E,H*C] or NULL), F.dropout(alpha, p) in training mode (:203), out[i,h] = sum_e alpha[e,h] v[src(e),h].
 * q, k, v [N,H*C] row-major; edge_index rows [source; target] `row_stride` apart (duplicate edges allowed); alpha [E,H] receives
 * the POST-softmax coefficients (what the operator returns), alpha_drop [E,H] the dropped ones (kept for the backward), out
 * [N,H*C].  Backward: dout [N,H*C] -> dq, dk, dv [N,H*C], dedge_feat [E,H*C] (NULL iff edge_feat is); ds_ws: E*H floats.
 * Deterministic: sums over a node's edges in edge order, fixed-tree block reductions.  Endpoints must lie in [0,N): the host
 * mirror validates each edge list once (IndexError, like the reference's index_select); the kernels clamp what they index with, so
 * a bad list gives unspecified coefficients for that edge, not a wild read.  E = 0 is legal (out = 0). */
int rd_edge_attention_fwd(int32_t N, int32_t E, int32_t H, int32_t C, const float* q, const float* k, const float* v,
                          const float* edge_feat, const int64_t* edge_index, int64_t row_stride, float p_drop, uint64_t seed,
                          float* alpha, float* alpha_drop, float* out, void* stream);
int rd_edge_attention_bwd(int32_t N, int32_t E, int32_t H, int32_t C, const float* q, const float* k, const float* v,
                          const float* edge_feat, const int64_t* edge_index, int64_t row_stride, float p_drop, uint64_t seed,
                          const float* alpha, const float* alpha_drop, const float* dout, float* ds_ws, float* dq, float* dk,
                          float* dv, float* dedge_feat, void* stream);

/* Batched forms (replace the per-sample Python loop + torch index_put_ the round-2 TransformerConv surface used):
 *  - rd_edge_softmax_list_batched: B edge lists in one launch, edge_index [B][2,E] int64 `batch_stride` elements apart (0 = one
 *    shared list), rows `row_stride` apart; weights [B,E] `w_bstride` floats apart (0 = shared); gamma_e [B,E], ssum [B,N].
 *    Layer 2 of the use_beta model reads each sample's OWN pruned edge list through it (code/models_rd.py:331-335).
 *  - rd_edge_gamma_dense: dense coefficient matrix gamma[j*N + i] = sum of gamma_e over the edges j -> i, duplicate edges added in
 *    edge order (the scatter-add of PyG's aggregate, code/transformer_conv.py:139-160, deterministic: no float atomics).
 *  - rd_aggregate_batched_fwd/bwd: out[b,i,c] = sum_j gamma[j,i] V[b,j,c] (+ skip[b,i,c]) for B feature matrices that share the
 *    graph, as ONE batched product (the legacy `Raindrop` model loops the operator over the batch, code/models_rd.py:155-165). */
int rd_edge_softmax_list_batched(int32_t B, int32_t N, int32_t E, const int64_t* edge_index, int64_t batch_stride,
                                 int64_t row_stride, int32_t norm_row, const float* edge_weights, int64_t w_bstride,
                                 float* gamma_e, float* ssum, void* stream);
/* rd_edge_softmax_list_batched followed by F.dropout(gamma, p) (what layer 2 of the use_beta model computes forward when its operator
 * was given dropout > 0, code/models_rd.py:331-336 -> code/Ob_propagation.py:196): gamma_e[b,e] is 0 or gamma / (1 - p), ssum the
 * sum of THOSE.  Forward only -- no gradient w.r.t. the weights is formed anywhere, which is why the model refuses that setting in
 * training mode: ssum no longer sums to 1 per target, so the weights' gradient is no longer 0.  The mask is
 * rd_edge_softmax_list_dropout's rule per (sample b, list position e): element e & 3 of quad b * ceil(E / 4) + e / 4 of the edge-
 * coefficient site under (seed + the registered seed cell).  p_drop = 0: rd_edge_softmax_list_batched. */
int rd_edge_softmax_list_batched_dropout(int32_t B, int32_t N, int32_t E, const int64_t* edge_index, int64_t batch_stride,
                                         int64_t row_stride, int32_t norm_row, const float* edge_weights, int64_t w_bstride,
                                         float p_drop, uint64_t seed, float* gamma_e, float* ssum, void* stream);
int rd_edge_gamma_dense(int32_t N, int32_t E, const int64_t* edge_index, int64_t row_stride, const float* gamma_e,
                        float* gamma_dense, void* stream);
int rd_aggregate_batched_fwd(int32_t B, int32_t N, int32_t C, const float* gamma, const float* V, const float* skip,
                             float* out, void* stream);
int rd_aggregate_batched_bwd(int32_t B, int32_t N, int32_t C, const float* gamma, const float* dout, float* dV, void* stream);

size_t rd_msgpass_workspace_bytes(const rd_shape* s);   /* scratch of rd_msgpass_bwd            */
size_t rd_msgpass_saved_bytes(const rd_shape* s);       /* forward -> backward hand-over buffer */

/* Forward of both Observation_progation layers for the whole batch
 * (code/models_rd.py:285-296,313-343 + code/Ob_propagation.py:157-228, default branch):
 *   X[b,f,t*d+c]  = relu(src[t,b,f] * R_u[f*d+c])            (observation embedding)
 *   Y1 = relu(X  W1^T + b1) * ssum[f];   Y2 = relu(Y1 W2^T + b2) * ssum[f]
 *   z[t,b,f*d+c]  = Y2[b,f,t*d+c]                            (columns [0, F*d) of z, row stride ldz)
 * src [T,B,2F] (values in the first F columns).  `saved` (rd_msgpass_saved_bytes) receives what
 * the backward pass needs: X and Y1 as [B,F,K] and the weights as split-bf16 operand tiles (fused path: its
 * planes; other shapes, bf16 modes: W1, W2, W2^T, W1^T as native tiles, 4 x 4 ceil16(K) ceil32(K) bytes).
 * p_drop > 0 applies nn.Dropout to the embedding h (code/models_rd.py:296) with a counter-based mask
 * that is a pure function of (seed, element index); p_drop = 0 in eval mode.
 * Shapes with F <= 48, d_ob = 4, K = T*d_ob <= 240, K % 16 == 0 (P19) run as ONE fused
 * LDS-resident kernel per batch (one workgroup per sample); others as two panel products (rd_gemm.hip:
 * k_gemm_panel) behind the observation-embedding kernel. */
int rd_msgpass_fwd(const rd_shape* s, const float* src, const float* R_u, const float* W1,
                   const float* b1, const float* W2, const float* b2, const float* ssum,
                   float p_drop, uint64_t seed, float* z, int32_t ldz, void* saved, size_t saved_bytes,
                   void* stream);

/* rd_pe_mask + rd_msgpass_fwd in one call for the model's layout (z [T,B,D], D = F*d_ob + d_pe,
 * contiguous; mask [B,T]).  On the fused path the positional encoding and the padding mask of a
 * sample are produced by the same workgroup that owns its message passing. */
int rd_sensor_stage_fwd(const rd_shape* s, const float* src, const float* times, const int64_t* lengths,
                        const float* timescales, const float* R_u, const float* W1, const float* b1,
                        const float* W2, const float* b2, const float* ssum, float p_drop, uint64_t seed,
                        float* z, uint8_t* mask, void* saved, size_t saved_bytes, void* stream);

/* rd_sensor_stage_fwd after rd_step_prepare has written this step's operand tiles of W1, W2 into `saved`: same arguments, same
 * results, no weight-split launch of its own. */
int rd_sensor_stage_fwd_prepared(const rd_shape* s, const float* src, const float* times, const int64_t* lengths,
                                 const float* timescales, const float* R_u, const float* W1, const float* b1,
                                 const float* W2, const float* b2, const float* ssum, float p_drop, uint64_t seed,
                                 float* z, uint8_t* mask, void* saved, size_t saved_bytes, void* stream);

/* Backward of rd_msgpass_fwd.  dz is the gradient w.r.t. z (row stride ldz; only the first
 * F*d columns are read).  Writes dW1,db1,dW2,db2 and dR_u [F*d] (overwrite, not accumulate). */
int rd_msgpass_bwd(const rd_shape* s, const float* src, const float* R_u, const float* W1,
                   const float* W2, const float* ssum, float p_drop, const void* saved,
                   size_t saved_bytes, const float* z, const float* dz, int32_t ldz, float* dW1,
                   float* db1, float* dW2, float* db2, float* dR_u, void* workspace,
                   size_t workspace_bytes, void* stream);

/* ---- coefficient dropout on the default branch (code/Ob_propagation.py:195-196 with use_beta = False) ------------------------
 * The reference calls each layer's operator once per sample and drops the post-softmax edge coefficients gamma [E,1] there: one
 * keep decision per (sample b, layer l, edge e), shared by all channels.  The value a coefficient multiplies is the TARGET's own,
 * so the layer's aggregate scale becomes
 *     s_l[b,i] = sum over the edges e into i of keep[b,l,e] / (1 - p_l) * softmax_i(w)[e]      (0 for a node without in-edges)
 * in place of ssum[i]:  Y1 = relu(X W1^T + b1) * s_1[b,f],  Y2 = relu(Y1 W2^T + b2) * s_2[b,f];  the backward's gates multiply by
 * the same numbers (dZ2 = dz * s_2 * (Y2 > 0), dZ1 = (dZ2 W2) * s_1 * (Y1 > 0)); the edge weights are no parameters, so nothing
 * else changes.
 *  - rd_msgpass_coef_table: coef [2][B][N] fp32 in ONE launch (one wave per (row, target), fixed-order sums, no atomics).  Row
 *    l * B + b is, bit for bit, row l * B + b of a 2B-row rd_edge_softmax_list_batched_dropout(batch_stride 0, w_bstride 0,
 *    norm_row 1, p_drop = p_l, seed) on the shared list (edge_index rows `row_stride` apart) -- the same mask rule, under seed +
 *    the registered seed cell (read when the kernel RUNS; the pointer is taken at enqueue); b is the sample's index in the CALLER's
 *    batch, with or without a token plan.  A layer with p_l = 0 gets `ssum` (rd_edge_softmax's).  Capturable.
 *  - the `_coef` entry points: their plain namesakes with the caller-owned table `coef` behind `ssum`; it is NOT part of `saved`
 *    (rd_msgpass_saved_bytes does not change) and is handed to rd_msgpass_bwd_coef again.  The plain entry points behave as
 *    coef == NULL.  The inference forward takes no table: evaluation never drops. */
int rd_msgpass_coef_table(int32_t B, int32_t N, int32_t E, const int64_t* edge_index, int64_t row_stride,
                          const float* edge_weights, const float* ssum, float p1, float p2, uint64_t seed, float* coef,
                          void* stream);
int rd_msgpass_fwd_coef(const rd_shape* s, const float* src, const float* R_u, const float* W1,
                        const float* b1, const float* W2, const float* b2, const float* ssum, const float* coef,
                        float p_drop, uint64_t seed, float* z, int32_t ldz, void* saved, size_t saved_bytes,
                        void* stream);
int rd_sensor_stage_fwd_coef(const rd_shape* s, const float* src, const float* times, const int64_t* lengths,
                             const float* timescales, const float* R_u, const float* W1, const float* b1,
                             const float* W2, const float* b2, const float* ssum, const float* coef, float p_drop,
                             uint64_t seed, float* z, uint8_t* mask, void* saved, size_t saved_bytes, void* stream);
int rd_sensor_stage_fwd_prepared_coef(const rd_shape* s, const float* src, const float* times, const int64_t* lengths,
                                      const float* timescales, const float* R_u, const float* W1, const float* b1,
                                      const float* W2, const float* b2, const float* ssum, const float* coef, float p_drop,
                                      uint64_t seed, float* z, uint8_t* mask, void* saved, size_t saved_bytes, void* stream);
int rd_msgpass_bwd_coef(const rd_shape* s, const float* src, const float* R_u, const float* W1,
                        const float* W2, const float* ssum, const float* coef, float p_drop, const void* saved,
                        size_t saved_bytes, const float* z, const float* dz, int32_t ldz, float* dW1,
                        float* db1, float* dW2, float* db2, float* dR_u, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ---- a15/a16: temporal self-attention encoder (kernels K2/K3) and masked mean (K5) --------- */

/* Parameters of one nn.TransformerEncoderLayer(D, nhead, nhid) (code/models_rd.py:235-237),
 * names as in its state_dict: self_attn.in_proj_{weight[3D,D],bias}, self_attn.out_proj.*,
 * linear1.{weight[nhid,D],bias}, linear2.{weight[D,nhid],bias}, norm1.*, norm2.* */
typedef struct rd_encoder_weights {
  const float *in_proj_w, *in_proj_b, *out_proj_w, *out_proj_b, *lin1_w, *lin1_b, *lin2_w, *lin2_b,
      *norm1_w, *norm1_b, *norm2_w, *norm2_b;
} rd_encoder_weights;
typedef struct rd_encoder_grads {
  float *in_proj_w, *in_proj_b, *out_proj_w, *out_proj_b, *lin1_w, *lin1_b, *lin2_w, *lin2_b,
      *norm1_w, *norm1_b, *norm2_w, *norm2_b;
} rd_encoder_grads;

size_t rd_encoder_layer_saved_bytes(const rd_shape* s);      /* activations kept for backward */
size_t rd_encoder_layer_workspace_bytes(const rd_shape* s);  /* scratch, fwd and bwd */

/* One post-norm encoder layer, torch semantics (torch/nn/modules/transformer.py:799-983, used at
 * code/models_rd.py:358): x,y [T,B,D] with D = F*d_ob + d_pe; mask [B,T] bytes (1 = padded key);
 * y = LN2(x1 + drop(W2 drop(relu(W1 x1)))) with x1 = LN1(x + drop(out_proj(MHA(x)))).
 * The four dropout sites use Philox masks keyed by (seed, site, layer). */
int rd_encoder_layer_fwd(const rd_shape* s, int32_t layer, const float* x, const uint8_t* mask,
                         const rd_encoder_weights* w, float p_drop, uint64_t seed, float* y,
                         void* saved, size_t saved_bytes, void* workspace, size_t workspace_bytes,
                         void* stream);
/* Optional: the weight-dependent part of the forward (splitting the layer's matrices into matrix-core operand tiles inside
 * `saved`) as its own call, for callers whose weights change less often than they run forward (inference: prepare once per
 * checkpoint); then pass `layer | RD_LAYER_WEIGHTS_PREPARED` to rd_encoder_layer_fwd, which skips that launch.  The caller
 * orders the two calls (same stream, or an event). */
#define RD_LAYER_WEIGHTS_PREPARED 0x10000
int rd_encoder_layer_prepare(const rd_shape* s, const rd_encoder_weights* w, void* saved, size_t saved_bytes,
                             void* stream);
/* Every weight matrix of a training step -> operand tiles in ONE launch (the weights change once per step, in the optimizer):
 * the `nlayers` (<= 2) encoder layers' into their `saved` buffers (what rd_encoder_layer_prepare does per layer) and the two
 * lin_value matrices of the message-passing stage into its `saved` buffer (what rd_sensor_stage_fwd does first; pass NULL to
 * skip).  Then call rd_encoder_layer_fwd(layer | RD_LAYER_WEIGHTS_PREPARED) and rd_sensor_stage_fwd_prepared.
 * rd_step_prepare_covers reports (1 / 0) whether the encoder layers / the sensor stage of this shape take prepared tiles in the
 * current arithmetic mode; where it says 0 the plain entry points must be used. */
int rd_step_prepare(const rd_shape* s, int32_t nlayers, const rd_encoder_weights* const* w, void* const* enc_saved,
                    const size_t* enc_saved_bytes, const float* W1, const float* W2, void* k1_saved, size_t k1_saved_bytes,
                    void* stream);
int rd_step_prepare_covers(const rd_shape* s, int32_t* encoder, int32_t* sensor_stage);
/* rd_token_plan and rd_step_prepare as ONE launch (the plan is built by one extra block row of the weight-split kernel: independent workgroups, a wave per sample): what a
 * hipGraph training step enqueues first.  seed_cell_dev / delta as in rd_token_plan (NULL: no bump). */
int rd_step_begin(const rd_shape* s, const int64_t* lengths, int32_t* plan_out, uint64_t* seed_cell_dev, uint64_t delta,
                  int32_t nlayers, const rd_encoder_weights* const* w, void* const* enc_saved, const size_t* enc_saved_bytes,
                  const float* W1, const float* W2, void* k1_saved, size_t k1_saved_bytes, void* stream);
/* Backward: dy -> dx and all 12 parameter gradients (overwritten). */
int rd_encoder_layer_bwd(const rd_shape* s, int32_t layer, const float* x, const uint8_t* mask,
                         const rd_encoder_weights* w, float p_drop, uint64_t seed, const void* saved,
                         size_t saved_bytes, const float* dy, float* dx, const rd_encoder_grads* g,
                         void* workspace, size_t workspace_bytes, void* stream);

/* The attention core of that layer alone (between in_proj and out_proj; torch F.multi_head_attention_forward as used at
 * code/models_rd.py:235-237,358): qkv [T,B,3D] (q | k | v, heads side by side) -> out [T,B,D] and lse [B,H,T] (log-sum-exp of the
 * scaled masked scores, consumed by the backward); backward dout [T,B,D] -> dqkv [T,B,3D] (delta_ws: B*H*T floats of scratch).
 * Same kernels as inside rd_encoder_layer_fwd/bwd (head_dim <= 96).  Dropout on the probabilities with Philox site
 * (attention, layer). */
int rd_attention_fwd(const rd_shape* s, int32_t layer, const float* qkv, const uint8_t* mask, float p_drop, uint64_t seed,
                     float* out, float* lse, void* stream);
int rd_attention_bwd(const rd_shape* s, int32_t layer, const float* qkv, const uint8_t* mask, float p_drop, uint64_t seed,
                     const float* out, const float* lse, const float* dout, float* dqkv, float* delta_ws, void* stream);

/* code/models_rd.py:366-367,379: out[b, :D] = sum_t r[t,b,:] * (1 - mask[b,t]) / (lengths[b] + 1);
 * out has row stride ldo (so it can be the left block of the [agg | emb] head input).  The forward follows a registered token
 * plan (r then holds the live rows only; same sums in the same order, so the same bits as on the padded layout); the backward
 * does not (the training step's plan runs the fused head). */
int rd_masked_mean_fwd(const rd_shape* s, int32_t D, const float* r, const uint8_t* mask,
                       const int64_t* lengths, float* out, int32_t ldo, void* stream);
int rd_masked_mean_bwd(const rd_shape* s, int32_t D, const float* dout, int32_t ldo,
                       const uint8_t* mask, const int64_t* lengths, float* dr, void* stream);

/* ---- caller step (a19): the optimizer of code/Raindrop.py:256 ------------------------------- */

/* torch.optim.Adam (no amsgrad; weight_decay added to the gradient) over one flat buffer of n floats, as ONE launch, in eight forms
 * (and their eight _grp twins further down: per-group learning rate and weight decay, coupled or decoupled):
 *     rd_adam_step [_clip] [_ema] [_dev]
 *   m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps),   g = grad + weight_decay * p.
 * Shared arguments: `n`; `param`, `grad`, `exp_avg`, `exp_avg_sq` (n floats each, 16-byte aligned); `beta1`, `beta2`, `eps` (launch
 * constants); `stream`.  The forms differ in where the step's scalars come from and in two optional riders:
 *   host forms (no _dev): `lr`, `weight_decay` and `step` = t (1-based) are arguments; the bias corrections are formed on the host.
 *   _dev: they are read from `state`, so the launch is one a hipGraph can replay.
 *   _clip: the gradient is scaled to a global norm first, and a non-finite gradient skips the step (`partial`, `partial_bytes`, `clip`).
 *   _ema: an exponential moving average of the parameters is kept by the same launch (`ema`, `ema_cell`).
 * The three cells are 64 bytes, 16-byte aligned, eight doubles each; a launch never reads a word another workgroup of the same
 * launch writes, and a value the caller may change between replays (lr, the threshold, the decay) is an 8-byte copy, not a new capture.
 *   `state` {t, beta1^t, beta2^t, lr, base lr, weight_decay, n, 0} OF THE STEP BEING APPLIED; the update only reads it (slots 0-3 and
 *     5).  It is advanced once per step by an EARLIER launch: rd_adam_state_advance (one thread: t += 1, beta^t *= beta), or -- no
 *     extra launch -- by the step's first launch: rd_set_adam_state registers the cell on this host thread and rd_step_begin
 *     (enqueued while it is registered) advances it next to the dropout seed bump.  Initialise {steps taken so far, beta1^t,
 *     beta2^t, lr, 0, wd, 0, 0}.  (A per-epoch schedule, code/Raindrop.py:257-259, writes slot 3.)
 *     Per-step schedule: slot 6 = n > 0 makes the state 8 + capacity doubles (n <= capacity), a table of factors f[0 .. n) from
 *     double 8 on; the advancing thread then also writes slot 3 = slot 4 * f[min(t - 1, n - 1)] with the t it has just formed (one
 *     double product; the last factor holds past the end; a step the non-finite guard skips still moves the position).  With
 *     n == 0 -- the eight-double state above -- slot 3 is the caller's and slot 4 is not read.  The C entry points take no length:
 *     a caller that sets n > 0 guarantees the 8 + n doubles (raindrop_amd.optim.FlatAdam checks it on the host).
 *   `clip` {max_norm, last_norm, last_scale, skipped, clipped, 0, 0, 0}: slot 0 is read by the launch and written by the caller only
 *     (+inf: guard without clipping); slots 1-4 are written by one thread of the launch -- the norm and the scale it applied (0 when
 *     it skipped) and two running counts of skipped / clipped steps.
 *   `ema_cell` {d, warm-up, k0, k1, 0, 0, 0, 0}: slot 0 the decay d, slot 1 the warm-up flag (0 or 1), both the caller's.  Slots 2 and
 *     3 hold k, the number of EMA updates so far, and belong to the launch: with s the step number (`step` of the host forms; t of
 *     `state` for the _dev forms) every workgroup reads k from slot 2 + (s & 1) and one thread writes k + 1 to slot 2 + ((s + 1) & 1)
 *     -- no atomics, two replays from the same state give the same bits.  The caller initialises BOTH slots to the count (0), and
 *     again whenever it makes the step number jump (steps must follow each other by one for the parity to select the slot last written).
 * RD_EINVAL before any launch: a NULL or misaligned pointer, step < 1, n <= 0, partial_bytes < rd_grad_sumsq_bytes().  One exception:
 * plain rd_adam_step accepts n == 0 and returns RD_OK without a launch; the seven other forms refuse it.
 * raindrop_amd.optim.FlatAdam.step / step_captured; raindrop_amd.step.TrainStep.capture_full. */
int rd_adam_step(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr,
                 float beta1, float beta2, float eps, float weight_decay, int64_t step, void* stream);
int rd_adam_step_dev(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float beta1, float beta2,
                     float eps, const void* state, void* stream);
int rd_adam_state_advance(void* state, float beta1, float beta2, void* stream);
int rd_set_adam_state(void* state, float beta1, float beta2);      /* NULL: unregister */

/* _clip: global-norm gradient clipping and the non-finite guard, torch.nn.utils.clip_grad_norm_ between backward and the update, as
 * two launches a hipGraph can hold (raindrop_amd.optim.FlatAdam(max_grad_norm=...)).
 * rd_grad_sumsq: partial[w] = sum of grad[i]^2 over the w-th of rd_grad_sumsq_grid() contiguous slices, squared and accumulated in
 * double in a fixed order (no atomics: the same bits on every launch).  `partial`: rd_grad_sumsq_bytes() bytes, 16-byte aligned.
 * The update then: every workgroup sums the partials in index order, norm = sqrt(sum), scale = norm > max_norm ? max_norm /
 * (norm + 1e-6) : 1 (clip_grad_norm_'s coefficient, clamped at 1), then Adam with g = grad * scale + weight_decay * p.  A sum that is
 * not finite (an inf or NaN gradient) makes the launch store NOTHING: param, exp_avg, exp_avg_sq keep their bits.  At scale == 1 the
 * update is that of the form without _clip, bit for bit.  The step state of the _dev form is advanced as always, skipped or not. */
int32_t rd_grad_sumsq_grid(void);
size_t rd_grad_sumsq_bytes(void);
int rd_grad_sumsq(int64_t n, const float* grad, void* partial, size_t partial_bytes, void* stream);
int rd_adam_step_clip(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                      float beta2, float eps, float weight_decay, int64_t step, const void* partial, size_t partial_bytes,
                      void* clip, void* stream);
int rd_adam_step_clip_dev(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float beta1, float beta2,
                          float eps, const void* state, const void* partial, size_t partial_bytes, void* clip, void* stream);

/* _ema: the exponential moving average of the weights inside the update's own launch (raindrop_amd.optim.FlatAdam(ema_decay=...)):
 * the four forms above with `ema` (n floats, 16-byte aligned) and `ema_cell` in front of the stream.  After the Adam update of
 * element i, in fp32, in the thread that wrote p_new:  ema[i] += c_t * (p_new[i] - ema[i]),  c_t = 1 - d_t rounded to float once, d_t
 * formed in double by every workgroup: d_t = d, or with warm-up min(d, (1 + k) / (10 + k)) (k: 0-based; not the number of steps).
 * param, exp_avg, exp_avg_sq get the bits of the form without _ema.  A step the clip forms skip stores nothing to `ema` and writes
 * k, not k + 1: the skipped step is no update of the average. */
int rd_adam_step_ema(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                     float beta2, float eps, float weight_decay, int64_t step, float* ema, void* ema_cell, void* stream);
int rd_adam_step_ema_dev(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float beta1, float beta2,
                         float eps, const void* state, float* ema, void* ema_cell, void* stream);
int rd_adam_step_clip_ema(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                          float beta2, float eps, float weight_decay, int64_t step, const void* partial, size_t partial_bytes,
                          void* clip, float* ema, void* ema_cell, void* stream);
int rd_adam_step_clip_ema_dev(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float beta1,
                              float beta2, float eps, const void* state, const void* partial, size_t partial_bytes, void* clip,
                              float* ema, void* ema_cell, void* stream);
/* _grp: parameter groups and decoupled weight decay (raindrop_amd.optim.FlatAdam(groups=..., decoupled=...)): the eight forms above
 * with `chunk_group` and `group_cell` in front of the stream.
 *   `chunk_group`: ceil(n / 64) bytes of device memory; byte c is the group id (0..15) of elements [64c, 64c + 64).  The caller lays
 *     the buffer out so that no 64-element chunk holds elements of two groups (raindrop_amd.dp.FlatGradAllReduce starts every tensor
 *     on a multiple of 64; the padding behind a tensor takes its group).  The launch uses `byte & 15`: no map indexes outside the cell.
 *   `group_cell`: 16 rows of four doubles {lr_scale, wd_coupled, wd_decoupled, 0}, 512 bytes, 16-byte aligned.  The launch only reads
 *     it; the caller writes a row with one 32-byte copy (not a new capture), as it writes slot 0 of the clip and EMA cells.
 * Element i of group r, with lr the `lr` argument (host forms) or slot 3 of `state` (_dev forms):
 *     lr_r = (float)((double)lr * lr_scale[r]);   p *= (float)(1 - (double)lr_r * wd_decoupled[r])      (torch.optim.AdamW's decay)
 *     g = grad * scale + (float)wd_coupled[r] * p;  m, v as above;  p -= lr_r / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
 * `scale` (_clip) stays that of the GLOBAL norm over all groups, the step count, the bias corrections and the EMA coefficient are
 * shared by all groups, and a skipped step stores nothing in any group.  `weight_decay` of the host forms and slot 5 of `state` are
 * NOT read: the caller resolves every group's decay into its row.  A row {1, wd, 0, 0} gives the bits of the form without _grp.
 * RD_EINVAL in addition to the twin's: NULL `chunk_group` / `group_cell`, a misaligned `group_cell`, n <= 0 (all eight forms). */
int rd_adam_step_grp(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                     float beta2, float eps, float weight_decay, int64_t step, const uint8_t* chunk_group, const void* group_cell,
                     void* stream);
int rd_adam_step_grp_dev(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float beta1, float beta2,
                         float eps, const void* state, const uint8_t* chunk_group, const void* group_cell, void* stream);
int rd_adam_step_clip_grp(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                          float beta2, float eps, float weight_decay, int64_t step, const void* partial, size_t partial_bytes,
                          void* clip, const uint8_t* chunk_group, const void* group_cell, void* stream);
int rd_adam_step_clip_grp_dev(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float beta1,
                              float beta2, float eps, const void* state, const void* partial, size_t partial_bytes, void* clip,
                              const uint8_t* chunk_group, const void* group_cell, void* stream);
int rd_adam_step_ema_grp(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                         float beta2, float eps, float weight_decay, int64_t step, float* ema, void* ema_cell,
                         const uint8_t* chunk_group, const void* group_cell, void* stream);
int rd_adam_step_ema_grp_dev(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float beta1,
                             float beta2, float eps, const void* state, float* ema, void* ema_cell, const uint8_t* chunk_group,
                             const void* group_cell, void* stream);
int rd_adam_step_clip_ema_grp(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                              float beta2, float eps, float weight_decay, int64_t step, const void* partial, size_t partial_bytes,
                              void* clip, float* ema, void* ema_cell, const uint8_t* chunk_group, const void* group_cell,
                              void* stream);
int rd_adam_step_clip_ema_grp_dev(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float beta1,
                                  float beta2, float eps, const void* state, const void* partial, size_t partial_bytes, void* clip,
                                  float* ema, void* ema_cell, const uint8_t* chunk_group, const void* group_cell, void* stream);
/* a <-> b over n floats in place (16-byte accesses, a scalar tail; capturable): FlatAdam.swap_ema exchanges the flat parameters and
 * their average, so that whatever holds the parameters' addresses evaluates the average.  a, b: 16-byte aligned, not overlapping.
 * RD_EINVAL: NULL or misaligned pointers, n <= 0. */
int rd_swap_f32(int64_t n, float* a, float* b, void* stream);
/* Gradient accumulation over a window of k micro-batches (raindrop_amd.step.TrainStep(accumulate=k)): two fp32 element-wise launches
 * over the flat gradient buffer `g` and an accumulator `acc` of n floats each, capturable, without atomics, the same bits on every
 * launch.
 *   rd_grad_accumulate:        acc[i] = acc[i] + g[i]                                   (the micro-batches of a window but the last)
 *   rd_grad_accumulate_close:  g[i] = (acc[i] + g[i]) * s;  acc[i] = 0                  (the last: `g` holds the window's mean)
 * `s` is the one float at `scale_cell` (device memory, 4-byte aligned), read when the kernel RUNS: 1/k, or 1/j for a window cut short
 * after j micro-batches -- a 4-byte copy between replays, not a new capture.  One fp32 add, then one fp32 multiply, both rounded to
 * nearest on their own (never fused): torch's `(acc + g) * s` bit for bit.  inf / NaN in `g` or `acc` propagate into `g`; `acc` is
 * +0 after the close whatever it held, so a poisoned window reaches the update's non-finite guard (_clip) and the next one starts clean.
 * 16-byte accesses with a scalar tail for n % 4; nothing at or behind element n is read or written.  g, acc: 16-byte aligned, not
 * overlapping.  RD_EINVAL: NULL or misaligned pointers, n < 0; n == 0 is RD_OK without a launch. */
int rd_grad_accumulate(int64_t n, const float* g, float* acc, void* stream);
int rd_grad_accumulate_close(int64_t n, float* g, float* acc, const float* scale_cell, void* stream);

/* ---- generic dense pieces (used by the temporal encoder, the head and the large-K path) ---- */

/* y[M,N] = act(x[M,K] W[N,K]^T + b)   (torch.nn.functional.linear; act: 0 none, 1 relu). */
int rd_linear_fwd(int32_t M, int32_t N, int32_t K, const float* x, int32_t ldx, const float* W,
                  const float* b, float* y, int32_t ldy, int32_t act, void* stream);
/* The same product on the exact-fp32 matrix instruction whatever the process's arithmetic mode (rd_set_precision): for values that
 * feed index work (code/Ob_propagation.py:161-185: edge scores -> top-K pruning).  Affects this call only, on this host thread. */
int rd_linear_fwd_fp32(int32_t M, int32_t N, int32_t K, const float* x, int32_t ldx, const float* W,
                       const float* b, float* y, int32_t ldy, int32_t act, void* stream);
/* dx[M,K] = dy[M,N] W[N,K]   (optionally masked by relu_src > 0 when relu_src != NULL). */
int rd_linear_bwd_input(int32_t M, int32_t N, int32_t K, const float* dy, int32_t lddy,
                        const float* W, float* dx, int32_t lddx, void* stream);
/* dx = (dy W) where gate[m,k] > 0, else 0: the ReLU of nn.Sequential(Linear, ReLU, Linear)
 * (mlp_static, code/models_rd.py:254-258) folded into the input-gradient product. */
int rd_linear_bwd_input_gated(int32_t M, int32_t N, int32_t K, const float* dy, int32_t lddy,
                              const float* W, const float* gate, int32_t ldgate, float* dx, int32_t lddx,
                              void* stream);
/* torch.nn.CrossEntropyLoss() (mean) forward + backward in one launch (code/Raindrop.py:255,322):
 * loss[0] = mean_b(logsumexp(logits[b]) - logits[b, y[b]]); dlogits = (softmax - onehot) / B. */
int rd_softmax_xent(int32_t B, int32_t C, const float* logits, const int64_t* y, float* loss,
                    float* dlogits, void* stream);
/* torch.nn.CrossEntropyLoss(weight = w, label_smoothing = eps) (mean) forward + backward in one launch, any C.
 * crit = [eps, w_0 .. w_{C-1}] (C + 1 floats on the device, read when the kernel runs); p = softmax(logits[b]), W = sum_b w[y[b]]:
 *   loss[0]      = (1 - eps) sum_b w[y_b] (-log p[b,y_b]) / W + (eps / C) sum_b sum_c w_c (-log p[b,c]) / W
 *   dlogits[b,c] = (1 - eps) (w[y_b] / W) (p[b,c] - [c == y_b]) + (eps / C) (1 / W) (p[b,c] sum_k w_k - w_c)
 * W is formed from per-class label counts, sum over c ascending of n_c w_c: the same bits in every launch (and in every workgroup
 * of rd_head_train_crit).  With eps = 0 and every w_c = 1 loss and dlogits are rd_softmax_xent's bit for bit.  W == 0 gives NaN (as
 * torch); a label outside [0, C) gives a NaN loss and reads nothing out of bounds.  B < 2^24. */
int rd_softmax_xent_crit(int32_t B, int32_t C, const float* logits, const int64_t* y, const float* crit, float* loss,
                         float* dlogits, void* stream);
/* The focal loss (Lin et al., "Focal Loss for Dense Object Detection") with class weights, forward + backward in one launch, any C.
 * crit = [gamma, w_0 .. w_{C-1}] (C + 1 floats on the device, read when the kernel runs; gamma finite in [0, 16], w_c >= 0);
 * p = softmax(logits[b]), logp_y = logits[b,y_b] - logsumexp(logits[b]), W = sum_b w[y_b]:
 *   q_b          = sum over c != y_b, ascending, of p[b,c]        (NOT 1 - p[b,y_b]: no cancellation when p[b,y_b] -> 1)
 *   m_b          = q_b^gamma                                      (gamma == 0: exactly 1; q_b == 0 and gamma > 0: exactly 0)
 *   g_b          = m_b - gamma p[b,y_b] q_b^(gamma - 1) logp_y    (gamma == 0: exactly 1; q_b == 0 and gamma > 0: exactly 0; the
 *                                                                   second term exactly 0 where logp_y has rounded to 0: never 0 * inf)
 *   loss[0]      = sum_b w[y_b] m_b (-logp_y) / W
 *   dlogits[b,c] = (p[b,c] - [c == y_b]) g_b w[y_b] / W
 * W is rd_softmax_xent_crit's (per-class label counts, sum over c ascending of n_c w_c) and so is the order of the factors: with
 * gamma = 0 loss and dlogits are rd_softmax_xent_crit's at eps = 0 bit for bit (CrossEntropyLoss(weight = w); the plain mean at
 * w = 1).  W == 0 gives NaN; a label outside [0, C) gives a NaN loss and reads nothing out of bounds.  B < 2^24. */
int rd_softmax_xent_focal(int32_t B, int32_t C, const float* logits, const int64_t* y, const float* crit, float* loss,
                          float* dlogits, void* stream);
/* Tuning knob of the encoder's row-block products (process-global, read when a product is enqueued): bit mask of the kernel
 * variants that run on 32-row instead of 64-row workgroups (1: K <= 160, 2: K <= 288, 4: LayerNorm epilogue, 8: LayerNorm-
 * backward prologue); -1 restores the default (environment RD_RG_ROWS32, else 15).  Results do not depend on it beyond
 * the grouping of the LayerNorm parameter-gradient partial sums.  raindrop_amd.step.TrainStep times both settings when
 * it captures its graph and keeps the faster one. */
int rd_set_rowgemm_rows32(int32_t mask);
/* Same bit assignment: kernel variants that run on 16-wave (1024-thread) workgroups, one column tile per wave and round, instead
 * of 8-wave ones; -1 restores the default (environment RD_RG_WAVES16, else 12). */
int rd_set_rowgemm_waves16(int32_t mask);
/* Classifier head + loss, forward and backward, in two launches (training step; rd_head.hip).
 *   agg = masked mean over time of r [T,B,D] (code/models_rd.py:366-367,379); feat = [agg | static W_emb^T + b_emb]
 *   (:381-384; Fe = 0: no static branch); logits = W2 relu(W0 feat + b0) + b2 (mlp_static, :263-267,385);
 *   loss = mean cross entropy against y (code/Raindrop.py:255,322).
 * Outputs: loss[1], logits [B,C], the six parameter gradients (overwritten, not accumulated) and dr [T,B,D], the
 * gradient entering the encoder stack.  fp32 FMA arithmetic in every precision mode.  Replaces the sequence
 * rd_masked_mean_fwd, rd_linear_fwd x3, rd_softmax_xent, rd_linear_bwd_weight x3, rd_linear_bwd_input(_gated),
 * rd_masked_mean_bwd of the same quantities.  rd_head_train_supported: D % 4 == 0, D + Fe <= 256, C <= 16 (and the
 * environment switch RD_HEAD_FUSED=0 reports 0); workspace: rd_head_train_workspace_bytes(B, D + Fe, C). */
int rd_head_train_supported(int32_t D, int32_t Fe, int32_t C);
size_t rd_head_train_workspace_bytes(int32_t B, int32_t dh, int32_t C);
int rd_head_train(const rd_shape* s, int32_t D, int32_t d_static, int32_t Fe, int32_t C, const float* r,
                  const uint8_t* mask, const int64_t* lengths, const float* stat, const float* emb_w,
                  const float* emb_b, const float* w0, const float* b0, const float* w2, const float* b2,
                  const int64_t* y, float* loss, float* logits, float* g_emb_w, float* g_emb_b, float* g_w0,
                  float* g_b0, float* g_w2, float* g_b2, float* dr, void* workspace, size_t workspace_bytes,
                  void* stream);
/* rd_head_train with rd_softmax_xent_crit's loss (class weights and label smoothing; crit = [eps, w_0 .. w_{C-1}] on the device,
 * read when the kernels run: a captured step changes its criterion by a copy into that buffer) in place of the plain mean cross
 * entropy.  Same two launches, support test and workspace as rd_head_train (criterion instantiations of its first kernel; every
 * workgroup forms W itself from the labels, in the fixed order above: no atomics, the same bits in every launch).  With eps = 0
 * and every w_c = 1: logits, dr and the six parameter gradients are rd_head_train's bit for bit.  B < 2^24. */
int rd_head_train_crit(const rd_shape* s, int32_t D, int32_t d_static, int32_t Fe, int32_t C, const float* r,
                       const uint8_t* mask, const int64_t* lengths, const float* stat, const float* emb_w,
                       const float* emb_b, const float* w0, const float* b0, const float* w2, const float* b2,
                       const int64_t* y, const float* crit, float* loss, float* logits, float* g_emb_w, float* g_emb_b,
                       float* g_w0, float* g_b0, float* g_w2, float* g_b2, float* dr, void* workspace, size_t workspace_bytes,
                       void* stream);
/* rd_head_train with rd_softmax_xent_focal's loss (crit = [gamma, w_0 .. w_{C-1}] on the device, read when the kernels run: a
 * captured step changes gamma and the weights by a copy into that buffer).  rd_head_train_crit's argument list, support test and
 * workspace; focal instantiations of its first kernel on the same label count and W -- no atomics, the same bits in every launch.
 * With gamma = 0: loss, logits, dr and the six parameter gradients are rd_head_train_crit's at eps = 0 bit for bit.  B < 2^24. */
int rd_head_train_focal(const rd_shape* s, int32_t D, int32_t d_static, int32_t Fe, int32_t C, const float* r,
                        const uint8_t* mask, const int64_t* lengths, const float* stat, const float* emb_w,
                        const float* emb_b, const float* w0, const float* b0, const float* w2, const float* b2,
                        const int64_t* y, const float* crit, float* loss, float* logits, float* g_emb_w, float* g_emb_b,
                        float* g_w0, float* g_b0, float* g_w2, float* g_b2, float* dr, void* workspace, size_t workspace_bytes,
                        void* stream);
/* The same head around a loss the CALLER evaluates -- the reference's loop: outputs = model(..); loss = criterion(outputs, y);
 * loss.backward() (code/Raindrop.py:317-323).  rd_head_forward stops at the logits; rd_head_backward recomputes the head's
 * forward phases (a masked mean and two small products) and continues from the caller's d loss / d logits [B,C].  Same kernel,
 * arithmetic, support test and workspace as rd_head_train.  raindrop_amd.graph_module (the captured module step) uses them. */
int rd_head_forward(const rd_shape* s, int32_t D, int32_t d_static, int32_t Fe, int32_t C, const float* r, const uint8_t* mask,
                    const int64_t* lengths, const float* stat, const float* emb_w, const float* emb_b, const float* w0,
                    const float* b0, const float* w2, const float* b2, float* logits, void* workspace, size_t workspace_bytes,
                    void* stream);
int rd_head_backward(const rd_shape* s, int32_t D, int32_t d_static, int32_t Fe, int32_t C, const float* r, const uint8_t* mask,
                     const int64_t* lengths, const float* stat, const float* emb_w, const float* emb_b, const float* w0,
                     const float* b0, const float* w2, const float* b2, const float* dlogits, float* g_emb_w, float* g_emb_b,
                     float* g_w0, float* g_b0, float* g_w2, float* g_b2, float* dr, void* workspace, size_t workspace_bytes,
                     void* stream);
size_t rd_linear_bwd_weight_workspace_bytes(int32_t M, int32_t N, int32_t K);
/* dW[N,K] = dy[M,N]^T x[M,K];  db[N] = sum_m dy[m,:]  (db may be NULL).  Deterministic split
 * over M with a fixed-order reduction. */
int rd_linear_bwd_weight(int32_t M, int32_t N, int32_t K, const float* dy, int32_t lddy,
                         const float* x, int32_t ldx, float* dW, float* db, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ---- batch feed: the caller's per-step slice, code/Raindrop.py:310-317 ---------------- */

/* `P = Ptrain_tensor[:, idx, :]`, `Ptime = Ptrain_time_tensor[:, idx]`, `Pstatic = Ptrain_static_tensor[idx]`,
 * `y = ytrain_tensor[idx]` (host fancy-index + H2D in the reference, :310-315) and
 * `lengths = torch.sum(Ptime > 0, dim=0)` (:317) in ONE launch over a dataset that is resident in HBM:
 * P_all [T,N,W] (W = 2F), time_all [T,N], static_all [N,d_static] or NULL, y_all [N] or NULL, idx [B] int64
 * (device) -> src [T,B,W], times [T,B], static_out [B,d_static], y_out [B], lengths [B] int64.  Pure copies:
 * bit-exact.  An index outside [0,N) is clamped and ADDED to *bad_index_count (device int32, may be NULL; the
 * caller zeroes it -- the library enqueues nothing but the one kernel). */
int rd_batch_gather(int32_t T, int32_t B, int32_t W, int32_t d_static, int64_t N, const float* P_all,
                    const float* time_all, const float* static_all, const int64_t* y_all, const int64_t* idx,
                    float* src, float* times, float* static_out, int64_t* y_out, int64_t* lengths,
                    int32_t* bad_index_count, void* stream);

/* The batch of a captured step from a device-resident EPOCH PLAN (raindrop_amd.feed.EpochFeed): rd_batch_gather with
 * idx = plan[cursor], where plan is int64 [capacity, B] and cell = int64[2] {cursor, n_batches} are read ON THE DEVICE when
 * the kernel runs (the cursor through the scalar cache: it is uniform) -- a replay of the same hipGraph gathers the next
 * batch, and a new epoch is a copy into plan and cell, never a new capture.  Writes src, times, static_out, y_out and lengths
 * exactly as rd_batch_gather(idx = plan[cursor]) does, bit for bit; y_all / y_out are required.  Nothing outside the plan is
 * ever read: n_batches is cut to capacity, and a cursor outside [0, n_batches) reads the last valid row (row 0 of an empty
 * plan) and adds ONE to *bad_index_count; sample indices outside [0,N) are clamped and counted as in rd_batch_gather.  The
 * cell is not written (rd_feed_record advances it).  Asynchronous, capturable; B == 0 is a no-op. */
int rd_feed_gather(int32_t T, int32_t B, int32_t W, int32_t d_static, int64_t N, int64_t capacity, const float* P_all,
                   const float* time_all, const float* static_all, const int64_t* y_all, const int64_t* plan,
                   const int64_t* cell, float* src, float* times, float* static_out, int64_t* y_out, int64_t* lengths,
                   int32_t* bad_index_count, void* stream);
/* rd_batch_gather / rd_feed_gather with TRAIN-TIME INPUT AUGMENTATION in the same launch (raindrop_amd.feed.Augment; DESIGN 3e').
 * W must be even: W = 2F, columns [0,F) values, [F,2F) observed-indicators (odd W: RD_EINVAL).  aug_cell: 32 bytes on the device,
 * 8-byte aligned, {u64 seed, u64 epoch, f32 p_time, f32 p_sensor, f32 p_obs, f32 noise_c}, read when the kernel RUNS (new rates, a
 * new epoch: a copy, never a new capture).  Every decision is a pure function of key = seed + draw (uint64, wrapping) and SOURCE
 * coordinates: the uniform of element idx at site s is component idx & 3 of the generator's quad idx >> 2, keep iff u >= p.
 * draw = epoch * capacity + cursor (the plan row actually read) in the feed form; the explicit-index form takes `draw` by value and
 * ignores the cell's epoch.  With b the batch slot and t the row of the source sample, in this order:
 *   1. time-step drop, site 80, element b*T + t: candidates are the rows t < L, L = #{t : time[t] > 0}; a sample whose candidates
 *      would all be dropped keeps all of them.  Rows written: the kept candidates in order, the source rows [L,T) unchanged, then
 *      rows of +0.0 -- src and times alike; lengths[b] = #{written times > 0};
 *   2. sensor drop, site 81, element b*F + f: value and indicator +0.0 in every row of the sample;
 *   3. observation drop, site 82, element (t*B + b)*F + f: value and indicator +0.0;
 *   4. jitter, site 83, the four uniforms u of the WHOLE quad (t*B + b)*F + f, where the indicator is still non-zero:
 *      v' = fmaf(((u.x + u.y) + (u.z + u.w)) - 2, noise_c, v), noise_c = float(sqrt(3) * sigma): zero mean, deviation sigma.
 * A rate of exactly 0 draws nothing for its transform; all four at 0 write the plain twin's bytes.  Index clamping, the `bad`
 * counter, the cursor rules, labels and statics are the plain twins'.  One launch; asynchronous, capturable; B == 0 is a no-op. */
int rd_batch_gather_aug(int32_t T, int32_t B, int32_t W, int32_t d_static, int64_t N, const float* P_all,
                        const float* time_all, const float* static_all, const int64_t* y_all, const int64_t* idx,
                        float* src, float* times, float* static_out, int64_t* y_out, int64_t* lengths,
                        int32_t* bad_index_count, const void* aug_cell, uint64_t draw, void* stream);
int rd_feed_gather_aug(int32_t T, int32_t B, int32_t W, int32_t d_static, int64_t N, int64_t capacity, const float* P_all,
                       const float* time_all, const float* static_all, const int64_t* y_all, const int64_t* plan,
                       const int64_t* cell, float* src, float* times, float* static_out, int64_t* y_out, int64_t* lengths,
                       int32_t* bad_index_count, const void* aug_cell, void* stream);
/* The LAST launch of a fed step (one workgroup), k = cursor: loss_hist[k] = *loss; correct_hist[k] = the number of samples b
 * with argmax_c logits[b, c] == y[b] (logits [B,C] row-major; ties go to the lowest class, a NaN is the maximum: torch.argmax;
 * int32, integer partial sums in a fixed order, no atomics); then cursor = k + 1.  loss_hist / correct_hist hold `capacity`
 * entries.  With the cursor outside [0, min(n_batches, capacity)) nothing is written and the cell stays as it is.  The cursor
 * is read by the step's first launch (rd_feed_gather) and advanced by this one: stream order inside one graph is the whole
 * protocol.  Asynchronous, capturable; B == 0 is a no-op. */
int rd_feed_record(int32_t B, int32_t C, int64_t capacity, int64_t* cell, const float* loss, const float* logits,
                   const int64_t* y, float* loss_hist, int32_t* correct_hist, void* stream);

/* ---- paper-faithful graph operator: the use_beta branch of Observation_progation.message,
 * code/Ob_propagation.py:161-185,190-191,195,200,207-208,227, batched over B sample graphs that share an edge list.
 *   V [B,N,K] = relu(lin_value(x)),  H [B,N,T*32] = increase_dim(x)   (both per NODE: rd_linear_fwd)
 *   beta[i,t] = mean_c H[i,t,c] * cat(map_weights[i], p_t[t])[c];  gamma[e,t] = beta[tgt(e),t] * w[e]
 *   keep the int(E*0.5) edges with the largest mean score, in descending order (ties: lower edge id first);
 *   softmax of gamma per channel over the kept edges of one SOURCE node;  out[n] = sum_{kept e: src(e)=n} softmax[e] (.) V[tgt(e)]
 * edge_index int64, rows [source; target] `row_stride` apart; edge_weights [E] per sample (stride w_bstride floats, 0 =
 * shared); p_t [T,16] per sample (stride pt_bstride floats, 0 = shared).  Outputs: out [B,N,K]; edge_index_out
 * [B][2,Kk] int64 and alpha_out [B][Kk] (the pruned edges in pruning order and their mean scores: what the reference
 * returns as (self.edge_index, self._alpha)), Kk = rd_graph_beta_kept(E); beta_save [B,N,T] and kept int32 [B,Kk] are
 * handed to the backward.  d_ob must be 4.  Two forms behind the same entry points: graphs with N <= 64 nodes and E <= 4096 edges
 * whose per-step scores fit one workgroup's LDS run as ONE launch per direction (graph staged in LDS); anything larger, up to
 * N <= 1024 nodes and 2^28 edges (round 4: SYN256's 256 sensors x 65 536 edges x 512 steps), runs as a sequence of
 * element-parallel launches with the per-sample state -- sort keys, kept-edge lists by source and by target, softmax statistics
 * -- in `workspace` (256-byte aligned, rd_graph_beta_workspace_bytes(..) bytes, 0 where the LDS form applies: then the two
 * workspace arguments are ignored).  Same pruning order (descending score, ties by edge id) and the same order of every sum in
 * both forms.  The reference has no limit (code/Ob_propagation.py:161-185). */
int32_t rd_graph_beta_kept(int32_t E);
size_t rd_graph_beta_workspace_bytes(int32_t B, int32_t N, int32_t K, int32_t T, int32_t E);
int rd_graph_beta_fwd(int32_t B, int32_t N, int32_t K, int32_t T, int32_t d_ob, int32_t E, const float* V, const float* H,
                      const float* map_weights, const float* p_t, int64_t pt_bstride, const int64_t* edge_index,
                      int64_t row_stride, const float* edge_weights, int64_t w_bstride, float* out, int64_t* edge_index_out,
                      float* alpha_out, float* beta_save, int32_t* kept, void* workspace, size_t workspace_bytes, void* stream);
/* Backward: dout [B,N,K] -> dV [B,N,K], dH [B,N,T*32], dmap_part [B,N,16] (sum over B = d map_weights), dw [B,E] or NULL. */
int rd_graph_beta_bwd(int32_t B, int32_t N, int32_t K, int32_t T, int32_t d_ob, int32_t E, const float* V, const float* H,
                      const float* map_weights, const float* p_t, int64_t pt_bstride, const int64_t* edge_index,
                      int64_t row_stride, const float* edge_weights, int64_t w_bstride, const float* beta_save,
                      const int32_t* kept, const float* dout, float* dV, float* dH, float* dmap_part, float* dw, void* workspace,
                      size_t workspace_bytes, void* stream);
/* rd_graph_beta_bwd with a second cotangent: dalpha [B,Kk], the gradient that arrives at alpha_out (the structure distance's,
 * code/models_rd.py:345-346; the reference's alpha is differentiable).  With alpha[b,q] = (1/T) sum_t beta[b,tgt,t] * w[b,e]
 * (e = kept[b,q]) it adds dbeta[b,n,t] += (1/T) sum_{q: tgt = n} dalpha[b,q] w[b,e] -- the same for every t, carried on to dH and
 * dmap_part like the rest of dbeta -- and dw[b,e] += dalpha[b,q] (1/T) sum_t beta[b,tgt,t].  dalpha NULL: exactly
 * rd_graph_beta_bwd.  Both forms (LDS-staged and workspace); the rounds 2-5 kernels (env RD_BETA_V1=1) refuse a non-NULL dalpha
 * with RD_EUNSUPPORTED.  No atomics: two calls give the same bits. */
int rd_graph_beta_bwd_alpha(int32_t B, int32_t N, int32_t K, int32_t T, int32_t d_ob, int32_t E, const float* V, const float* H,
                            const float* map_weights, const float* p_t, int64_t pt_bstride, const int64_t* edge_index,
                            int64_t row_stride, const float* edge_weights, int64_t w_bstride, const float* beta_save,
                            const int32_t* kept, const float* dout, const float* dalpha, float* dV, float* dH, float* dmap_part,
                            float* dw, void* workspace, size_t workspace_bytes, void* stream);
/* Coefficient dropout of the use_beta branch: F.dropout(gamma, p) after the softmax (code/Ob_propagation.py:195-196).  The reference
 * repeats gamma to [E/2, T*d_ob] before the softmax and drops element-wise, so the d_ob = 4 channels of one (edge, step) share the
 * softmax weight P and have four independent keep decisions:
 *   out[b,s,4t+c] = sum over kept e with src(e) = s of  P[b,e,t] * keep[b,e,t,c] / (1 - p) * V[b,tgt(e),4t+c]
 * THE MASK: one quad of the library's counter-based generator per (sample b, edge e, step t) at the edge-coefficient site, under
 * (seed + the registered seed cell, read at enqueue), its four uniforms the four channels, keep iff u >= p:
 *   quad = (b * E + e) * T + t,  e = the edge's id in the INPUT list (not its position among the kept ones)
 * so both forms, both directions and every sample draw from one numbering (< 2^48 at every supported size).  Only the aggregation
 * sees the mask: pruning, edge_index_out, alpha_out (the reference saves _alpha before the softmax), beta_save and kept do not
 * depend on p.  The backward regenerates the mask from (p_drop, seed) -- pass the forward's; nothing more is stored --:
 *   dV[b,g,4t+c] += P keep / (1 - p) dout[b,s,4t+c],  dP[b,e,t] = sum_c keep / (1 - p) dout[b,s,4t+c] V[b,g,4t+c],
 * then the softmax backward and the rest as in rd_graph_beta_bwd; the dalpha path (NULL allowed) does not see the mask.  Fixed
 * order of every sum, no atomics: two calls give the same bits.  p_drop = 0 runs rd_graph_beta_fwd / _bwd(_alpha) themselves.  Both
 * forms; the rounds 2-5 kernels (env RD_BETA_V1=1) refuse p_drop > 0 with RD_EUNSUPPORTED.
 * rd_graph_beta_keep writes that mask for EVERY edge of the input list: keep [B,E,T,4] bytes (1 = kept), through the same device
 * function the kernels call. */
int rd_graph_beta_fwd_dropout(int32_t B, int32_t N, int32_t K, int32_t T, int32_t d_ob, int32_t E, const float* V, const float* H,
                              const float* map_weights, const float* p_t, int64_t pt_bstride, const int64_t* edge_index,
                              int64_t row_stride, const float* edge_weights, int64_t w_bstride, float p_drop, uint64_t seed,
                              float* out, int64_t* edge_index_out, float* alpha_out, float* beta_save, int32_t* kept,
                              void* workspace, size_t workspace_bytes, void* stream);
int rd_graph_beta_bwd_dropout(int32_t B, int32_t N, int32_t K, int32_t T, int32_t d_ob, int32_t E, const float* V, const float* H,
                              const float* map_weights, const float* p_t, int64_t pt_bstride, const int64_t* edge_index,
                              int64_t row_stride, const float* edge_weights, int64_t w_bstride, float p_drop, uint64_t seed,
                              const float* beta_save, const int32_t* kept, const float* dout, const float* dalpha, float* dV,
                              float* dH, float* dmap_part, float* dw, void* workspace, size_t workspace_bytes, void* stream);
int rd_graph_beta_keep(int32_t B, int32_t T, int32_t E, float p_drop, uint64_t seed, uint8_t* keep, void* stream);
/* code/models_rd.py:345-346: distance = mean(cdist(alpha_all.T, alpha_all.T, p=2)) for alpha_all [E,B] (one column of edge
 * scores per sample); workspace B floats.  Identically 0 on the shipped path (equal columns); evaluated here in general. */
int rd_structure_distance(int32_t E, int32_t B, const float* alpha_all, float* workspace, float* distance, void* stream);
/* Its backward: grad = the device scalar d loss / d distance (read on the device: capturable) -> dalpha_all [E,B],
 *   dalpha_all[e,b] = sum_c C[b,c] (alpha_all[e,b] - alpha_all[e,c]),  C[b,c] = 2 grad / (B^2 D[b,c]),  D[b,c] = ||column b - column c||,
 * C = 0 where D = 0 (torch's cdist convention: B = 1 and identical columns give exact zeros, no NaN).  Any E (0 included) and B;
 * fp32, fixed-order sums, no atomics.  workspace: rd_structure_distance_bwd_workspace_bytes(E, B) bytes (B*B floats, 4-byte
 * aligned), caller-owned. */
size_t rd_structure_distance_bwd_workspace_bytes(int32_t E, int32_t B);
int rd_structure_distance_bwd(int32_t E, int32_t B, const float* alpha_all, const float* grad, void* workspace, size_t workspace_bytes,
                              float* dalpha_all, void* stream);

/* ---- building blocks of the paper-faithful sensor stage: Raindrop_v2(use_beta=True), i.e. code/models_rd.py:313-343 with the
 * literal at :317 flipped.  Layer 1 prunes a different edge set per sample, so the stage is composed instead of fused:
 *   rd_obs_embed_fwd -> rd_linear_fwd (lin_value + ReLU, increase_dim) -> rd_graph_beta_fwd -> rd_edge_softmax_list_batched ->
 *   rd_linear_fwd (layer 2's lin_value + ReLU) -> rd_rows_to_tokens_fwd; rd_pe_mask writes the PE columns and the mask.
 *  - rd_obs_embed_fwd: X[b,f,t*d+c] = dropout(relu(src[t,b,f] * R_u[f*d+c]))  ([B,F,T*d]; code/models_rd.py:290-296,326-327; same
 *    dropout site and element numbering as the fused stage).  rd_obs_embed_bwd: dR_u from dX (gate X > 0 = ReLU open AND kept).
 *  - rd_rows_to_tokens_fwd: z[t,b,f*d+c] = Y[b,f,t*d+c] * rowscale[b,f] (rowscale NULL = 1): the aggregate coefficient of layer 2
 *    (sum of the per-target softmax over a sample's surviving edges) and the layout change of code/models_rd.py:338-342;
 *    _bwd: dY = dz * rowscale in Y's layout. */
/* Scalar scale + nn.Dropout as a pure function of (seed + seed cell, site, element index): out = x * scale * keep / (1 - p)
 * (p = 0: the plain scale).  The backward is the same call on the gradient.  Sites < 16 are free for callers (the library's own sites start at 16; the observation embedding is 1).
 * The legacy `Raindrop` model's `encoder(src) * sqrt(d_model)` and input dropout (code/models_rd.py:131-134) run through it. */
int rd_scale_dropout(int64_t n, const float* x, float scale, float p_drop, uint64_t seed, uint32_t site, float* out, void* stream);

int rd_obs_embed_fwd(const rd_shape* s, const float* src, const float* R_u, float p_drop, uint64_t seed, float* X, void* stream);
size_t rd_obs_embed_bwd_workspace_bytes(const rd_shape* s);
int rd_obs_embed_bwd(const rd_shape* s, const float* src, const float* X, const float* dX, float p_drop, float* dR_u,
                     void* workspace, size_t workspace_bytes, void* stream);
int rd_rows_to_tokens_fwd(const rd_shape* s, const float* Y, const float* rowscale, float* z, int32_t ldz, void* stream);
int rd_rows_to_tokens_bwd(const rd_shape* s, const float* dz, int32_t ldz, const float* rowscale, float* dY, void* stream);

/* ---- the use_beta sensor stage as ONE pair in the training step's layout (raindrop_amd/step_beta.py BetaTrainStep) ----------
 * What Raindrop_v2._sensor_stage_beta composes under autograd (code/models_rd.py:313-346 with `use_beta` on), enqueued by the library:
 * PE + mask, observation embedding (its dropout site), V = relu(lin_value(X)), H = increase_dim(X) in exact fp32 in every arithmetic
 * mode (it feeds the top-K), rd_graph_beta_fwd, layer 2's relu(lin_value(y1)), the per-sample aggregate coefficient and the
 * [B,F,T*d] -> [T,B,F*d | PE] layout.  z follows the token plan registered by rd_set_token_plan (live rows only) or is the padded
 * [T,B,D]; the seed cell is read at enqueue like rd_sensor_stage_fwd does.  Asynchronous, capturable, caller-owned memory only.
 * Needs d_ob = 4, d_pe = 16, F <= 1024.  edge_index int64 rows [source; target] `row_stride` apart, edge_weights [E] (shared).
 * Outputs: z, mask [B,T], edge_index_out [B][2,Kk] int64, alpha_out [B,Kk] (Kk = rd_graph_beta_kept(E)), and, when `distance` is
 * not NULL, the structure distance (rd_structure_distance of alpha_out^T).  `saved` (rd_beta_stage_saved_bytes) goes to the
 * backward; `workspace` (rd_beta_stage_workspace_bytes, one size for both directions) is scratch.  256-byte aligned both.
 * Backward: dz (row stride lddz, the forward's layout) -> the gradients of R_u, both lin_value pairs, increase_dim.weight / .bias
 * and map_weights, WRITTEN (not accumulated) into the given destinations.  dist_grad: device scalar lambda of CE + lambda * distance
 * (rd_structure_distance_bwd -> rd_graph_beta_bwd_alpha); NULL: rd_graph_beta_bwd exactly as the autograd surface runs it.  The
 * backward forms what the distance's gradient needs from `alpha` itself: it does not matter whether the forward was given a
 * `distance` destination. */
size_t rd_beta_stage_workspace_bytes(const rd_shape* s, int32_t E);
size_t rd_beta_stage_saved_bytes(const rd_shape* s, int32_t E);
int rd_beta_stage_fwd(const rd_shape* s, const float* src, const float* times, const int64_t* lengths, const float* timescales,
                      const float* R_u, const float* W1, const float* b1, const float* Winc, const float* binc,
                      const float* map_weights, const float* W2, const float* b2, const int64_t* edge_index, int64_t row_stride,
                      const float* edge_weights, int32_t E, float p_drop, uint64_t seed, float* z, uint8_t* mask,
                      int64_t* edge_index_out, float* alpha_out, float* distance, void* saved, size_t saved_bytes, void* workspace,
                      size_t workspace_bytes, void* stream);
int rd_beta_stage_bwd(const rd_shape* s, const float* src, const float* R_u, const float* W1, const float* Winc,
                      const float* map_weights, const float* W2, const int64_t* edge_index, int64_t row_stride,
                      const float* edge_weights, int32_t E, float p_drop, const int64_t* edge_index_kept, const float* alpha,
                      const void* saved, size_t saved_bytes, const float* dz, int32_t lddz, const float* dist_grad, float* dR_u,
                      float* dW1, float* db1, float* dWinc, float* dbinc, float* dmap_weights, float* dW2, float* db2,
                      void* workspace, size_t workspace_bytes, void* stream);
/* The pair with coefficient dropout on layer 1's operator (Raindrop_v2(use_beta=True) whose ob_propagation.dropout was set; training
 * mode): p_edge1 drops layer 1's post-softmax coefficients (rd_graph_beta_fwd_dropout under `seed` + the registered seed cell); the
 * backward takes p_edge1 and the forward's seed and regenerates the mask.  p_edge1 = 0: rd_beta_stage_fwd / _bwd exactly.
 * Layer 2's coefficient dropout is NOT built into the stage: with it the per-target coefficient sum no longer equals 1 and the
 * edge scores get a gradient through it (d coef / d alpha), which no backward here forms; the model and the steps refuse
 * ob_propagation_layer2.dropout > 0 in training mode. */
int rd_beta_stage_fwd_dropout(const rd_shape* s, const float* src, const float* times, const int64_t* lengths, const float* timescales,
                              const float* R_u, const float* W1, const float* b1, const float* Winc, const float* binc,
                              const float* map_weights, const float* W2, const float* b2, const int64_t* edge_index, int64_t row_stride,
                              const float* edge_weights, int32_t E, float p_drop, float p_edge1, uint64_t seed, float* z,
                              uint8_t* mask, int64_t* edge_index_out, float* alpha_out, float* distance, void* saved,
                              size_t saved_bytes, void* workspace, size_t workspace_bytes, void* stream);
int rd_beta_stage_bwd_dropout(const rd_shape* s, const float* src, const float* R_u, const float* W1, const float* Winc,
                              const float* map_weights, const float* W2, const int64_t* edge_index, int64_t row_stride,
                              const float* edge_weights, int32_t E, float p_drop, float p_edge1, uint64_t seed,
                              const int64_t* edge_index_kept, const float* alpha, const void* saved, size_t saved_bytes,
                              const float* dz, int32_t lddz, const float* dist_grad, float* dR_u, float* dW1, float* db1,
                              float* dWinc, float* dbinc, float* dmap_weights, float* dW2, float* db2, void* workspace,
                              size_t workspace_bytes, void* stream);
/* The stage's two layout kernels on their own.  _fwd: z[row(t,b), f*4+c] = y2[b,f,t*4+c] * coef[b,f], coef = the per-target softmax
 * sum over sample b's kept edges (edge_index_kept [B][2,Kk], alpha [B,Kk]): bit-identical to rd_edge_softmax_list_batched(norm_row
 * = 1)'s ssum followed by rd_rows_to_tokens_fwd on the padded layout; with a token plan registered only the live rows are written,
 * at the plan's rows.  _bwd: dY[b,f,t*4+c] = dz[row(t,b), f*4+c] * coef[b,f] * (y2[b,f,t*4+c] > 0); steps without a row in the plan
 * layout get exact zeros.  16-byte aligned tensors, row strides multiples of 4.  coef_out (optional): the forward also stores coef
 * [B,F]; coef (optional): the backward reads that table instead of forming the softmax sums again (same bits; the stage does
 * this through `saved`).  The lists may be NULL when Kk = 0 (a graph of fewer than two edges keeps none: coef = 0). */
int rd_beta_l2_tokens_fwd(const rd_shape* s, int32_t Kk, const int64_t* edge_index_kept, const float* alpha, const float* y2, float* z,
                          int32_t ldz, float* coef_out, void* stream);
int rd_beta_l2_tokens_bwd(const rd_shape* s, int32_t Kk, const int64_t* edge_index_kept, const float* alpha, const float* y2,
                          const float* dz, int32_t lddz, const float* coef, float* dY, void* stream);

/* ---- inference forward: the forward of the model's stages without the save-for-backward buffers ---------------------------------
 * The training forwards above write, next to their results, what only a backward reads (row tiles and gate bits of the sensor stage;
 * pre-norm sums, statistics, FFN hidden / gate bytes, row tiles and the log-sum-exp of an encoder layer; X .. coef of the use_beta
 * stage).  The entry points here produce the SAME z / mask / y / kept edges / alpha / distance, bit for bit (dropout off: inference
 * never drops), and write none of that.  `saved` is then ONE smaller buffer per stage, rd_*_infer_bytes: the forward's weight operand
 * tiles and what one forward launch hands to the next.
 *  - rd_infer_covers: 1 / 0 per stage -- the shape has save-free kernel instantiations in the current arithmetic mode and switches
 *    (sensor stage: the fused message passing at the P19 shape; encoder: the fused row-local chain at the P19 widths on the
 *    row-block path, with the fused in_proj + attention launch on a token plan and the attention kernels of the training forward on
 *    the padded layout).  Where it says 0 the size query returns the training size and the entry point runs the saving forward into
 *    that buffer.  The use_beta stage has an inference form at every shape it supports.
 *  - A buffer of the inference size is carved differently from a training one; rd_encoder_layer_prepare, rd_step_prepare and
 *    rd_step_begin follow the SAME rule as the forward -- a buffer too small for the training carve holds the inference carve, and
 *    then receives the forward's tiles only --, so pass them the size you pass the forward.
 *  - rd_sensor_stage_fwd_infer: `prepared` != 0 after rd_step_prepare / rd_step_begin wrote this step's tiles (rd_sensor_stage_fwd_prepared's
 *    contract).  rd_encoder_layer_fwd_infer honours RD_LAYER_WEIGHTS_PREPARED; where rd_infer_covers says 1 it does not touch
 *    `workspace` (NULL / 0 allowed).  rd_beta_stage_fwd_infer keeps its large intermediates in `workspace`
 *    (rd_beta_stage_workspace_bytes), which may be shared with any call that does not overlap it.
 *  - A buffer smaller than the query's size is RD_EINVAL before any launch.  Token plan and seed-cell registrations are read as in
 *    the training forwards (the seed cell is ignored: nothing drops). */
int rd_infer_covers(const rd_shape* s, int32_t* sensor_stage, int32_t* encoder);
size_t rd_msgpass_infer_bytes(const rd_shape* s);
size_t rd_encoder_layer_infer_bytes(const rd_shape* s);
size_t rd_beta_stage_infer_bytes(const rd_shape* s, int32_t E);
int rd_sensor_stage_fwd_infer(const rd_shape* s, const float* src, const float* times, const int64_t* lengths,
                              const float* timescales, const float* R_u, const float* W1, const float* b1, const float* W2,
                              const float* b2, const float* ssum, float* z, uint8_t* mask, void* saved, size_t saved_bytes,
                              int32_t prepared, void* stream);
int rd_encoder_layer_fwd_infer(const rd_shape* s, int32_t layer, const float* x, const uint8_t* mask, const rd_encoder_weights* w,
                               float* y, void* saved, size_t saved_bytes, void* workspace, size_t workspace_bytes, void* stream);
int rd_beta_stage_fwd_infer(const rd_shape* s, const float* src, const float* times, const int64_t* lengths, const float* timescales,
                            const float* R_u, const float* W1, const float* b1, const float* Winc, const float* binc,
                            const float* map_weights, const float* W2, const float* b2, const int64_t* edge_index, int64_t row_stride,
                            const float* edge_weights, int32_t E, float* z, uint8_t* mask, int64_t* edge_index_out, float* alpha_out,
                            float* distance, void* saved, size_t saved_bytes, void* workspace, size_t workspace_bytes, void* stream);

/* ---- host preprocessing on the device: code/utils_rd.py:149-257, code/Raindrop.py:215-231 ------------
 * Inputs are float64 (the reference's numpy arrays), outputs float32 (its torch.Tensor casts).  Every result is
 * bit-identical to the reference: elementwise steps use the same IEEE float64 operations in the same order, and the
 * statistics reproduce numpy's pairwise summation tree (raindrop_amd/csrc/rd_preprocess.hip). */

/* utils_rd.getStats (:149-161): P [NT, F] (any [N,T,F] flattened) -> mf [F], stdf [F] = mean / max(population std, 1e-7)
 * of the values > 0 of every sensor.  NT < 2^31. */
size_t rd_prep_stats_workspace_bytes(int64_t NT, int32_t F);
int rd_prep_stats(int64_t NT, int32_t F, const double* P, double* mf, double* stdf, void* workspace,
                  size_t workspace_bytes, void* stream);
/* utils_rd.mask_normalize (:164-175) + the float32 cast of tensorize_normalize (:232): P [N,T,F] f64 -> out f32 with the
 * normalised values in channels [0,F) and the observation mask in [F,2F).  layout 0: out [N,T,2F]; layout 1: out
 * [T,N,2F], i.e. the permute of code/Raindrop.py:232-238 fused into the store. */
int rd_prep_mask_normalize(int64_t N, int32_t T, int32_t F, const double* P, const double* mf, const double* stdf,
                           float* out, int32_t layout, void* stream);
/* utils_rd.mask_normalize_static (:206-219) + float32 cast: S [N,D] f64 -> out [N,D] f32. */
int rd_prep_static(int64_t N, int32_t D, const double* S, const double* ms, const double* ss, float* out, void* stream);
/* `torch.Tensor(P_time) / 60.0` (:235,253): minutes [N,T] f64 -> hours f32, [N,T] (layout 0) or [T,N] (layout 1). */
int rd_prep_time(int64_t N, int32_t T, const double* minutes, float* hours, int32_t layout, void* stream);
/* Setting 2 / 3 (code/Raindrop.py:215-231): zero k value channels of every sample of P f32 ([N,T,2F] layout 0 or
 * [T,N,2F] layout 1) in place; idx int32 [N,k] (per_sample = 1: the per-patient np.random.choice draws, made by the
 * host in the reference's order) or [k] (per_sample = 0: the same top-ranked set for every sample). */
int rd_prep_remove_features(int64_t N, int32_t T, int32_t F, float* P, const int32_t* idx, int32_t k, int32_t per_sample,
                            int32_t layout, void* stream);

/* ---- validation metrics on the device (code/Raindrop.py:348-370,385-401; raindrop_amd/csrc/rd_metrics.hip) -----------------
 * What the reference computes on the host every epoch with sklearn, where the logits are.  Asynchronous, capturable, caller-owned
 * memory only.
 *
 * rd_rank_metrics: scores f32 [N, C] with row stride ld (floats), y int64 [N].  For every column c the one-vs-rest ranking
 * statistics of scores[:, c] against (y == c) with sklearn's semantics -- thresholds are the DISTINCT score values, tied scores
 * (float32 equality; -0 == +0) form one group; tp / fp = cumulative counts at the end of a tie group in descending score order,
 * P positives, Q = N - P:
 *   auroc_num[c] = sum (fp - fp_prev)(tp + tp_prev)                 exact int64
 *   auroc[c]     = auroc_num[c] / (2 P Q)                           float64; NaN when P = 0 or Q = 0
 *   auprc[c]     = sum (tp - tp_prev) / P * tp / (tp + fp)          float64, summed in an order that is a function of N alone;
 *                                                                   0 when P = 0 (sklearn's value: recall := 1, precision 0)
 *   mean[0], mean[1] = plain means of auroc / auprc over the columns (NaN when a column is NaN)
 * = roc_auc_score(one_hot(y), scores, average=None / "macro") and average_precision_score of the same; binary tasks read column 1.
 * Labels outside [0, C) are negatives of every column.  NaN scores are not refused (no host sync): a NaN with the sign bit clear
 * ranks above +inf, one with it set below -inf, equal payloads tie.  1 <= N <= 2^22, 1 <= C <= 65535.
 * N <= 16384: one launch, one workgroup per column, keys sorted in LDS, no workspace.  Larger N: 16384-key chunks sorted in LDS
 * with global compare-exchange launches between them, through `workspace` (rd_rank_metrics_workspace_bytes, 8-byte aligned). */
size_t rd_rank_metrics_workspace_bytes(int64_t N, int32_t C);
int rd_rank_metrics(int64_t N, int32_t C, const float* scores, int64_t ld, const int64_t* y, double* auroc, double* auprc,
                    double* mean, int64_t* auroc_num, void* workspace, size_t workspace_bytes, void* stream);
/* counts int64 [C, C] (overwritten): counts[t][p] = rows with label t whose first maximum (np.argmax; a NaN is a maximum) is
 * column p.  Rows with a label outside [0, C) are not counted.  Accuracy and macro precision / recall / F1 follow from the C^2
 * integers on the host.  C <= 4096. */
int rd_confusion(int64_t N, int32_t C, const float* logits, int64_t ld, const int64_t* y, int64_t* counts, void* stream);

/* Bootstrap of the ranking statistics (raindrop_amd/csrc/rd_metrics_boot.hip): R resamples of the N rows, every column's
 * statistics on each, and a percentile summary -- how far one AUROC / AUPRC of a small split can be trusted.  A resample changes
 * the MULTIPLICITY of a sample, never the order of the scores: every column is sorted once, the R resamples are R weighted scans.
 * Asynchronous, capturable, caller-owned memory only, no floating-point atomics: two calls give the same bits.
 *
 * Resample rule.  Resample r in [0, R) draws N row indices with replacement over the ORIGINAL rows, the same draw for every column.
 * Draw k in [0, N) reads raw 32-bit word k & 3 of generator quad q = r * ceil(N / 4) + (k >> 2) of site 84 (SITE_BOOTSTRAP)
 * under the key `seed` alone (no seed cell).  One Threefry-2x32-13 call gives two words, so a quad is two calls: words 0, 1 are
 * (x0, x1) of the call with counter 2 q, words 2, 3 those of counter 2 q + 1 -- counter (low word, high word | 84 << 16), key (seed
 * low word, seed high word), as for the dropout sites.  The index is j = floor(word * N / 2^32) (the high half of the 32 x 32
 * product): row j is drawn with probability floor or ceil(2^32 / N) / 2^32, a relative bias of at most N / 2^32 (< 4e-6).
 * m_r[j] = number of draws that hit j; every row of m sums to N.
 *
 * Statistics.  For column c and resample r: rd_rank_metrics' statistics with sample j counted m_r[j] times -- tp / fp are the
 * cumulative WEIGHTED counts at the end of each tie group in descending score order (a group whose members all have multiplicity
 * 0 contributes nothing), the float32 key order, the tie rule, the NaN order and "a label outside [0, C) is a negative" as above;
 *   pos_b[r][c]       = P_r = sum_j m_r[j] (y_j == c),  Q_r = N - P_r
 *   auroc_num_b[r][c] = sum (fp - fp_prev)(tp + tp_prev)               exact int64
 *   auroc_b[r][c]     = auroc_num_b / (2 P_r Q_r)                      float64; NaN when P_r = 0 or Q_r = 0
 *   auprc_b[r][c]     = sum (tp - tp_prev) / P_r * tp / (tp + fp)      float64, summed in an order that is a function of N alone;
 *                                                                      0 when P_r = 0
 *   mean_b[r][0 .. 1] = plain means of auroc_b[r] / auprc_b[r] over the columns (NaN when a column is NaN)
 * = roc_auc_score / average_precision_score on the expanded resample scores[idx_r], y[idx_r].
 * Envelope: 1 <= N <= 16384 (one LDS sort per column; larger N is deliberately out of scope: the chunked sort of rd_rank_metrics
 * has no index-carrying form), 1 <= C <= 65535, 1 <= R <= 4096; outside it RD_EUNSUPPORTED.  `workspace`:
 * rd_rank_bootstrap_workspace_bytes (0 outside the envelope), 2-byte aligned: per column the N sorted samples as 16-bit codes.
 *
 * rd_rank_bootstrap_summary: summary f64 [2][C + 1][5]: metric (0 AUROC, 1 AUPRC) x (column 0 .. C - 1, then the macro mean from
 * mean_b) x {n_valid, mean, standard deviation (ddof = 1), lower, upper} over the n_valid non-NaN resamples; lower / upper =
 * numpy.percentile(valid, [100 alpha / 2, 100 (1 - alpha / 2)]) (linear interpolation on the ascending values, sorted in LDS).
 * Sums are float64 in a fixed order.  n_valid < 2: deviation and interval NaN; n_valid = 0: the mean too.  0 < alpha < 1.
 *
 * rd_rank_bootstrap_counts: the multiplicities themselves, counts u32 [nr][N] = m_r for r = r0 .. r0 + nr - 1 (0 <= r0,
 * r0 + nr <= R), by the device function the statistics use: the tests' handle on the resample rule. */
size_t rd_rank_bootstrap_workspace_bytes(int64_t N, int32_t C, int32_t R);
int rd_rank_bootstrap(int64_t N, int32_t C, const float* scores, int64_t ld, const int64_t* y, int32_t R, uint64_t seed,
                      double* auroc_b, double* auprc_b, int64_t* auroc_num_b, int64_t* pos_b, double* mean_b, void* workspace,
                      size_t workspace_bytes, void* stream);
int rd_rank_bootstrap_summary(int32_t R, int32_t C, const double* auroc_b, const double* auprc_b, const double* mean_b, double alpha,
                              double* summary, void* stream);
int rd_rank_bootstrap_counts(int64_t N, int32_t R, uint64_t seed, int32_t r0, int32_t nr, uint32_t* counts, void* stream);

/* Calibration (raindrop_amd/csrc/rd_metrics_calib.hip): whether a predicted 0.8 means 80 % -- the reliability table and its
 * summaries, and the temperature (Guo et al., 2017) that minimises the NLL of softmax(logits / T).  Asynchronous, capturable,
 * caller-owned memory only, no floating-point atomics, every sum float64 in an order that is a function of the shapes alone: two
 * calls give the same bits.  Argument errors RD_EINVAL before any launch; outside the envelope RD_EUNSUPPORTED, no CPU fallback.
 *
 * rd_calibration: logits f32 [N, C] with row stride ld (floats), y int64 [N]; `temperature` a DEVICE float64 (so a fit's result
 * feeds it without a sync; its element 0 is read; NULL: T = 1; T > 0 is the caller's business).  p = softmax(logits / T) in
 * float64, max-subtracted.  column = -1, top-label mode: confidence = max_c p, hit = (argmax == y), the argmax the FIRST maximum of
 * the row's logits (np.argmax).  column = c, one-vs-rest mode: confidence = p[:, c], hit = (y == c).
 * Bin rule.  M equal-width bins with the edges e_i = (double)i / (double)M; a confidence falls in bin i iff e_i < conf <= e_{i+1}
 * (closed on the right: 0.5 with M = 10 is bin 4, 1.0 the last bin), and a confidence of exactly 0 goes to bin 0.  A NaN
 * confidence (a NaN logit) enters no bin.
 *   counts  int64 [M][2]   {n_b, hits_b}, exact
 *   table   f64 [M][3]     {n_b, mean confidence, hit rate}; the last two NaN for an empty bin
 *   summary f64 [6]        0 ECE = sum_b (n_b / N) |hit rate_b - mean confidence_b|     1 MCE = the maximum of that gap over the
 *                          NON-EMPTY bins (0 when all are empty)     2 Brier     3 NLL = -mean log p[n, y_n], always of the full
 *                          softmax, whatever the column     4 hit rate = sum hits_b / N     5 mean confidence = sum of the binned
 *                          confidences / N
 * Brier.  Top-label mode: mean_n sum_c (p_nc - [y_n = c])^2.  Column mode: mean_n (p_nc - [y_n = c])^2 of that column alone
 * (sklearn's brier_score_loss).  A label outside [0, C) makes its row a miss whose NLL and Brier terms are NaN (not refused: that
 * would cost a sync, the NaN-scores rule of rd_rank_metrics).
 * Envelope: 1 <= N < 2^24, 2 <= C <= 64, 1 <= M <= 256.  ceil(N / rows per workgroup) <= 1024 workgroups of 256 threads leave
 * per-bin partials in `workspace` (rd_calibration_workspace_bytes, 0 outside the envelope; 8-byte aligned; the layout depends on N
 * and M alone), one finishing workgroup sums them in workgroup order.
 *
 * rd_fit_temperature: the scalar T that minimises NLL(T) = mean_n [logsumexp(z_n / T) - z_{n,y} / T], found in beta = 1 / T, where
 * the objective is convex: g(beta) = mean(E_p[z] - z_y) and h(beta) = mean(Var_p[z]) = g' >= 0, p = softmax(beta z).  Bracket
 * [1e-2, 1e2]; the start is beta = 1, whose sign of g says on which side the minimum lies; g at the bracket's end on that side
 * decides between an interior minimum and a stop at the end; then a safeguarded Newton iteration from beta = 1 -- a step that
 * leaves the bracket, has h <= 0 or does not halve the previous step is replaced by the bracket's midpoint, and the sign of g at
 * every new beta moves one end of the bracket there.  It stops when the step or the bracket is <= 1e-12 beta, when g is exactly 0,
 * or after 100 evaluations of (g, h), the two above included.
 *   result f64 [8]   0 T     1 beta     2 NLL at T = 1     3 NLL at T     4 evaluations of (g, h)     5 status     6 g at the end     7 0
 * Status.  0 interior minimum (constant rows, g = 0 at beta = 1: T = 1)     1 stopped at T = 1e-2: the rows are separable and the
 * NLL still falls     2 stopped at T = 1e2 (labels worse than chance)     3 the evaluation cap was reached     4 a non-finite
 * gradient was met (a NaN or infinite logit, a label outside [0, C)): T = 1, beta = 1 and NLL at T = NLL at 1 are written, so
 * nothing downstream is poisoned.
 * Envelope: 1 <= N <= 16384 (the bootstrap's), 2 <= C <= 64.  One launch of one 1024-thread workgroup; the logits are staged once in
 * LDS when N C 4 <= 159 KiB, else re-read from global memory every evaluation: the same bits either way. */
size_t rd_calibration_workspace_bytes(int64_t N, int32_t C, int32_t M);
int rd_calibration(int64_t N, int32_t C, const float* logits, int64_t ld, const int64_t* y, const double* temperature, int32_t column,
                   int32_t M, int64_t* counts, double* table, double* summary, void* workspace, size_t workspace_bytes, void* stream);
int rd_fit_temperature(int64_t N, int32_t C, const float* logits, int64_t ld, const int64_t* y, double* result, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RAINDROP_HIP_H */
