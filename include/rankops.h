/*
 * rankops.h — C ABI of the MI355X (gfx950) CTR feature-interaction engine.
 *
 * Every entry point takes plain device pointers, sizes and a hipStream_t passed
 * as `void*` (NULL = the default stream).  Nothing here knows about torch: the
 * Python host layer (the rankops Python package) binds these with ctypes, exactly as the
 * reference's `nn.Module.forward()` bodies would bind them.
 * All work is enqueued asynchronously on `stream`; no entry point allocates
 * device memory or synchronises, so every forward can be captured in a hipGraph.
 *
 * Return value: RK_OK (0) or an RK_ERR_* code; rk_last_error() gives the text.
 * Out-of-range embedding indices never fault: the row is read as zeros and
 * RK_FLAG_INDEX_OOB is raised in the device flag word (rk_error_flags), the
 * analogue of nn.Embedding's IndexError / device assert.
 *
 * Reference interfaces replaced (file:line in the reference snapshot):
 *   rk_concat_gather   nn.Embedding lookups + torch.cat       dcn.py:163-169, deepcrossing.py:148-155,
 *                                                            din.py:296-305,310, bst.py:218-224,243
 *   rk_dcn_cross       cross_layer() loop + output_layer part dcn.py:25-50,171-173,177-178
 *   rk_fm_gather       DeepFM first/second-order FM + concat deepfm.py:122-142
 *   rk_fm_pack_table, rk_fm_gather_packed  the same over one packed [V, pad4(D+1)] table per field
 *   rk_linear          nn.Linear (+BatchNorm1d eval, ReLU/LeakyReLU/Dice/PReLU, residual,
 *                      LayerNorm, sum/mean pooling, final Linear(*,1)+sigmoid) dcn.py:144-152,175-180;
 *                      deepfm.py:100-112,143-151; din.py:26-36,272-285,312-316; deepcrossing.py:25-42,161-162;
 *                      bst.py:59-64,73-75,86-90,203-214,238-247
 *   rk_din_attention   din_attention() with the history gathered from the table  din.py:42-84,300-305
 *   rk_din_attention_dense  din_attention(query, keys[B,T,H], keys_length, is_softmax)  din.py:42-84
 *   rk_dien_interest   DIEN's GRU + attention + AGRU/AUGRU with the history gathered from the table
 *                      DIEN/dien.py:198-229, custom_grucell.py:19-167, rnn.py:201-219
 *   rk_dien_interest_dense  the same over a dense history tensor keys[B,T,H]
 *   rk_dien_interest_train(_dense), rk_dien_interest_backward  the train forward that keeps the
 *                      states, and backprop through time of the recurrence   DIEN/dien.py:314-334
 *   rk_dien_aux_loss(_dense), rk_dien_aux_loss_backward, rk_dien_interest_backward_aux  the auxiliary
 *                      loss over the extractor states and its gradients      DIEN/dien.py:256-300
 *   rk_dien_extract(_dense), rk_dien_evolve  rk_dien_interest cut in two for request-level scoring:
 *                      the extractor once per history, attention + evolution once per candidate
 *   rk_dien_forward(_plan)  the whole DIEN eval forward (row gather, rk_dien_interest, fcn tail, head)
 *                      in one launch
 *   rk_dice_forward   Dice.forward() in eval (BatchNorm running statistics)           din.py:26-36
 *   rk_row_l2norm_mean DIN mini-batch-aware l2 term          din.py:318-322
 *   rk_afm_forward     AFM.forward()                         afm.py:92-119
 *   rk_bst_attention   BSTTransformer scores/mask/softmax/AV bst.py:73-84 (mask from seq_length, bst.py:228-229)
 *   rk_bst_attention_masked  the same with BSTTransformer.forward's key_padding_mask  bst.py:66-84
 *   rk_bst_forward_blocks  all BSTTransformer blocks + pooling, fused bst.py:66-91,224-241
 *   rk_bst_forward_blocks_packed  the same on pre-packed projection weights
 *   rk_linear_tiled    one wide MLP layer (2D-tiled)          deepfm.py:100-112 (first deep layer)
 *   rk_fm_linear_packed  the DeepFM front end in one launch: packed-table gather, fm1, fm2 and the
 *                      first deep layer (the deep input never reaches HBM)  deepfm.py:100-112,122-142
 *   rk_deepfm_forward  DeepFM.forward() in one launch at configs[1]'s shape   deepfm.py:121-151
 *   rk_cin_forward, rk_cin_pack_weight  xDeepFM's front end in one launch: row gather, first-order sum,
 *                      the Compressed Interaction Network, its pooling and output layer (the
 *                      reference lists the model, its script is not in the snapshot)
 *   rk_cin_forward_train, rk_cin_pack_weight_t, rk_cin_backward, rk_cin_wgrad  xDeepFM training:
 *                      the CIN forward keeping its maps, its data backward and weight gradients
 *   rk_mmoe_forward    MMoE (multi-gate mixture of experts) eval forward in one launch: row gather,
 *                      gates + softmax, experts with the mix in their last epilogue, towers, heads
 *                      (the reference lists the model, its script is not in the snapshot)
 *   rk_ple_forward     PLE (progressive layered extraction) eval forward in one launch: row gather, L
 *                      levels of task / shared experts and gates, towers, heads
 *   rk_esmm_forward    ESMM (entire space multi-task model) eval forward in one launch: row gather once
 *                      for all towers, towers, heads, the chain of probabilities
 *   rk_fibinet_interaction, rk_fibinet_forward  FiBiNET: SENET field attention and the bilinear
 *                      interaction as one launch, and the whole eval forward (row gather, first-order
 *                      sum, SENET, both bilinear layers, deep layers, head) in one launch (the
 *                      reference lists the model, its script is not in the snapshot)
 *   rk_eval_batch, rk_auc  evaluate(): loss / accuracy / AUC on the device  dcn.py:214-239
 *   rk_topk_segments, rk_topk_by_request, rk_grouped_auc  the best k candidates of each request and
 *                      the per-user AUC / GAUC on the device (no counterpart in the reference)
 *   rk_fwfm_forward    FwFM.forward()                        fwfm.py:114-139
 *   training (loss.backward() + optimizer.step() of the train() loops, dcn.py:196-201):
 *   rk_gemm            the Linear backward GEMMs (dX = dZ W, dW = dZ^T X, db)   dcn.py:147-150
 *   rk_gemm_wgrad      dW = dZ^T X, db over long reductions (one tile owner per row slab)
 *   rk_gemm_grouped, rk_gemm_wgrad_grouped   G same-shaped Linear backwards in one launch each
 *   rk_mmoe_forward_train, rk_mmoe_mix_backward, rk_mmoe_head_backward   MMoE training
 *   rk_ple_forward_train, rk_ple_mix_backward   PLE training: the train form of the one-launch forward
 *                      and the backward of one level's mixtures and gates ("Training")
 *   rk_esmm_forward_train, rk_esmm_loss, rk_esmm_joint_backward   ESMM training: the train form of the
 *                      one-launch forward, the entire-space loss with its analytic gradient, and the
 *                      fold of gradients at the joint probabilities onto the logits
 *   rk_logit_head_backward  output_layer + sigmoid backward      dcn.py:177-179
 *   rk_dcn_cross_backward   cross_layer backward w.r.t. x0        dcn.py:46-49
 *   rk_relu_backward   ReLU backward (residual_unit's outer ReLU) deepcrossing.py:41
 *   rk_embedding_backward   nn.Embedding dense weight gradient    dcn.py:131-138,163-166
 *   rk_embedding_backward_seq  the same for a [batch, T] behaviour sequence (runs pre-summed)
 *   rk_embedding_backward_sorted  the same for long, skewed index lists (behaviour sequences)
 *                      as a sorted segment-reduce                din.py:300-303, bst.py:224
 *   rk_adam_step       torch.optim.Adam step (all tensors, one launch)  dcn.py:275
 *   rk_sparse_adam_step  torch.optim.SparseAdam / LazyAdam step over sparse table gradients
 *                      (all tables of a step in one call)         dien.py:328
 *   rk_pack_blocks     the value rows of sparse table gradients out of dx, all tables in one launch
 *   rk_bn_act_train_forward / rk_bn_act_backward  Linear -> BatchNorm1d (train) -> ReLU -> Dropout
 *                      and its backward                       deepfm.py:100-109
 *   rk_fm_backward, rk_fm_combine_backward  FM and final_layer + sigmoid backward  deepfm.py:122-151
 *   rk_shard_fm_assemble, rk_shard_fm_backward_pack, rk_shard_unpack_grads  the table-sharded
 *                      DeepFM's train step around its all-to-alls (the sharding is this build's own)
 *   rk_rng_next, rk_dropout_mask  dropout stream counter / explicit mask
 *   rk_dice_train_forward / rk_dice_backward  Dice with batch statistics and its backward  din.py:26-36
 *   rk_prelu_train_forward / rk_prelu_backward  the activation='prelu' option (nn.PReLU)  din.py:277-279
 *   rk_din_att_cross, rk_din_att_pool_forward, rk_din_att_pool_backward, rk_din_cross_fold
 *                      din_attention() train forward pieces and backward   din.py:42-84
 *   rk_row_l2norm_backward  DIN mini-batch-aware l2 term backward           din.py:318-322
 *   rk_fwfm_backward   FwFM backward (embedding rows, pair weights, bias)  fwfm.py:114-139,150-156
 *   rk_afm_pairs, rk_afm_pool_forward, rk_afm_pool_backward, rk_afm_pair_fold
 *   rk_bst_add_pos, rk_bst_gather_pos, rk_bst_attn_train_forward / _backward, rk_bst_res_dropout_ln_forward,
 *   rk_linear_res_dropout_ln (projection + residual LayerNorm fused),
 *   rk_bst_ln_backward, rk_bst_pool_ln_backward, rk_bst_pos_backward, rk_bst_leaky_dropout,
 *   rk_bst_pool / _backward
 *                      BSTTransformer train forward (activations kept) and backward  bst.py:66-91,238-241
 *                      AFM train forward (activations kept) and backward  afm.py:92-119,173
 *   rk_bn_fold         BatchNorm1d eval affine (running stats) deepfm.py:105, din.py:31,281, bst.py:208
 */
#ifndef RANKOPS_H
#define RANKOPS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RK_ABI_VERSION 6

#define RK_OK 0
#define RK_ERR_INVALID 1     /* bad argument (shape, null pointer, limit) */
#define RK_ERR_LAUNCH 2      /* hipLaunch / hipGetLastError failure */
#define RK_ERR_RUNTIME 3     /* other HIP runtime failure */
#define RK_ERR_UNSUPPORTED 4 /* shape outside the implemented envelope */

#define RK_FLAG_INDEX_OOB 1u /* an embedding index was < 0 or >= table rows */

#define RK_ACT_NONE 0
#define RK_ACT_RELU 1
#define RK_ACT_LEAKY 2 /* LeakyReLU(slope) */
#define RK_ACT_DICE 3  /* Dice: a*(1-p)*x + p*x, p = sigmoid(x*act_scale + act_shift) */
#define RK_ACT_PRELU 4 /* PReLU(act_alpha) */

#define RK_MAX_SEGMENTS 64

/* One column block of a concatenated feature row.
 * Table segment (idx != NULL): out[b, out_col:out_col+dim] = src[idx[b*idx_stride]*src_ld : +dim]
 * Dense segment (idx == NULL): out[b, out_col:out_col+dim] = src[b*src_ld : +dim]           */
typedef struct rk_segment {
  const float* src;
  const int64_t* idx;
  int64_t idx_stride;
  int64_t src_ld;
  int64_t rows; /* table rows (bounds check); ignored for dense segments */
  int32_t dim;
  int32_t out_col;
} rk_segment;

/* Fused GEMM epilogue, applied in this order to z = x.W^T:
 *   z += bias[n]; z += residual[m, n] (+ residual_periodic[m % period, n]);
 *   z = z*pre_scale[n] + pre_shift[n];   (BatchNorm1d eval before the activation)
 *   z = act(z);
 *   z = z*post_scale[n] + post_shift[n]; (BatchNorm1d eval after the activation: DIN)
 * then the optional row epilogues (need the whole row in one workgroup, N <= 256):
 *   LayerNorm over n (ln_gamma/ln_beta, ln_eps);
 *   pool: pool_out[g, n] = sum over rows m of group g (pool_rows consecutive rows),
 *         divided by pool_len[g] when pool_mean;
 *   head: logit[m] = sum_n z[m,n]*head_w[n] + head_b[0] (+ head_partial[m]);
 *         DeepFM combine when fm1 != NULL: head_aux[m] = logit (deep logit),
 *         logit = final_w[0]*fm1[m] + final_w[1]*fm2[m] + final_w[2]*deep + final_b[0];
 *         head_prob[m] = sigmoid(logit).
 * y may be NULL when only row-epilogue outputs are wanted.                              */
typedef struct rk_epilogue {
  const float* bias;
  const float* residual;
  int64_t ld_residual;
  const float* residual_periodic;
  int32_t residual_period;
  const float* pre_scale;
  const float* pre_shift;
  int32_t act;
  float slope;
  const float* act_scale;
  const float* act_shift;
  const float* act_alpha;
  int32_t act_alpha_len;
  const float* post_scale;
  const float* post_shift;
  const float* ln_gamma;
  const float* ln_beta;
  float ln_eps;
  int32_t has_ln;
  float* pool_out;
  int64_t ld_pool;
  int32_t pool_rows;
  int32_t pool_mean;
  const int64_t* pool_len;
  const float* head_w;
  const float* head_b;
  const float* head_partial;
  const float* fm1;
  const float* fm2;
  const float* final_w;
  const float* final_b;
  float* head_logit;
  float* head_prob;
  float* head_aux;
} rk_epilogue;

/* One hidden layer of a fused MLP tail (rk_mlp_forward): y = act(x.W^T + bias) with the same
 * element-wise epilogue order as rk_epilogue; `residual` adds the input of the previous layer
 * (DeepCrossing's ReLU(x + L2(ReLU(L1 x))), deepcrossing.py:37-41).                        */
#define RK_MLP_MAX_LAYERS 8
typedef struct rk_mlp_layer {
  const float* w; /* [n, K] row-major */
  int64_t ldw;
  int32_t n;
  int32_t act;
  float slope;
  int32_t residual;
  const float* bias;
  const float* pre_scale;
  const float* pre_shift;
  const float* act_scale;
  const float* act_shift;
  const float* act_alpha;
  int32_t act_alpha_len;
  const float* post_scale;
  const float* post_shift;
  float* store; /* optional: this layer's activations also written to store[m * ld_store + n]
                   (the training forward keeps them for the backward) */
  int64_t ld_store;
} rk_mlp_layer;

/* ---- runtime ---- */
int32_t rk_abi_version(void);
/* Provenance of this build: "src=<sha256[:16] of the sources> arch=<gfx> extra=<flags>". */
const char* rk_build_info(void);
const char* rk_last_error(void);
int rk_init(int32_t device);
/* Reads (and optionally clears) the device flag word; synchronises the device. */
int rk_error_flags(int32_t device, uint32_t* flags, int32_t reset);

/* ---- embedding gather / interaction kernels ---- */
int rk_concat_gather(const rk_segment* segs, int32_t nseg, int64_t batch, float* out,
                     int64_t ld_out, void* stream);

/* x0 = concat(segs); x_0 = xl_in (or x0 when NULL); x_{l+1} = x0*(x_l.w_l) + b_l + x_l.
 * Optional outputs: x0 (the gathered row), xl_out (x_L), cross_partial = x_L.head_w.      */
int rk_dcn_cross(const rk_segment* segs, int32_t nseg, int64_t batch, int32_t width,
                 const float* cross_w, const float* cross_b, int32_t num_layers,
                 const float* head_w, float* x0, int64_t ld_x0, const float* xl_in,
                 int64_t ld_xl_in, float* xl_out, int64_t ld_xl_out, float* cross_partial,
                 void* stream);

/* Segments are either all embedding tables (idx != NULL) or all dense (row b of src); dim/4 a
 * power of two, dim <= 256, at most 32 fields. */
int rk_fm_gather(const rk_segment* second_order, const rk_segment* first_order,
                 int32_t num_fields, int32_t dim, int64_t batch, float* deep_in,
                 int64_t ld_deep, float* fm1, float* fm2, void* stream);

/* One field's DeepFM tables packed into one row-major [rows, ld_out] table (ld_out % 4 == 0,
 * ld_out >= dim + 1): second-order row at columns 0..dim-1, first-order weight at column dim,
 * zero padding.  Replaces the pair nn.Embedding(V, dim) + nn.Embedding(V, 1) of one field
 * (deepfm.py:90-98) as the storage the eval gather reads; a layout pass run once per weight
 * version (the host layer caches it like the packed MLP weights).                            */
int rk_fm_pack_table(const float* second, int64_t ld_second, const float* first, int64_t ld_first,
                     int64_t rows, int32_t dim, float* out, int64_t ld_out, void* stream);

/* rk_fm_gather over packed tables (deepfm.py:122-142): segment f = {packed table of field f,
 * its [B] int64 indices (unit stride), src_ld = the packed row stride, rows, dim, out_col}.  One
 * contiguous row read per (sample, field) gives both embedding orders.                          */
int rk_fm_gather_packed(const rk_segment* fields, int32_t num_fields, int32_t dim, int64_t batch,
                        float* deep_in, int64_t ld_deep, float* fm1, float* fm2, void* stream);

int rk_din_attention(const float* query, int64_t ld_query, const float* key_table,
                     int64_t key_rows, int64_t ld_key, const int64_t* seq, int64_t ld_seq,
                     int32_t T, const int64_t* seq_len, int64_t batch, int32_t H,
                     const float* w1, const float* b1, const float* w2, const float* b2,
                     const float* w3, const float* b3, int32_t use_softmax, float* out,
                     int64_t ld_out, void* stream);

/* din_attention(query, keys, keys_length, is_softmax) with a dense history tensor: key row t of
 * sample b at keys + b * ld_keys_b + t * ld_keys_t (16-B aligned rows).  H in {8,16,32,64}.   */
int rk_din_attention_dense(const float* query, int64_t ld_query, const float* keys, int64_t ld_keys_b,
                           int64_t ld_keys_t, int32_t T, const int64_t* keys_length, int64_t batch,
                           int32_t H, const float* w1, const float* b1, const float* w2,
                           const float* b2, const float* w3, const float* b3, int32_t use_softmax,
                           float* out, int64_t ld_out, void* stream);

/* DIEN interest extractor + interest evolution, eval forward, one launch (DIEN/dien.py:198-229):
 *   h_t   = GRUCell(x_t, h_{t-1}), x_t = key_table[seq[b, t]], h_{-1} = 0  (TF GRUCell: [r|u] =
 *           sigmoid([x, h] Wg^T + bg), c = tanh([x, r*h] Wc^T + bc), h_t = u*h + (1-u)*c)
 *   a     = softmax over all T positions of s_t = h_t . (A query[b]), s_t = -2^32+1 for t >= seq_len[b]
 *   s_t   = AGRU (cell_type 0: (1-a_t)*s + a_t*c) or AUGRU (cell_type 1: u' = (1-a_t)*u,
 *           u'*s + (1-u')*c) over the inputs h_t with weights Vg / Vc, t < seq_len[b] only
 *   out[b, 0:nh] = s after step seq_len[b]-1 (zeros when seq_len[b] == 0);
 *   att_out[b, 0:T] = a when att_out != NULL (uniform 1/T when seq_len[b] == 0).
 * Weights, row-major: Wg [2nh, H+nh] (r rows first, then u), bg [2nh], Wc [nh, H+nh], bc [nh],
 * A [nh, H], Vg [2nh, 2nh], vg [2nh], Vc [nh, 2nh], vc [nh].  query row b at query + b*ld_query and
 * out row b at out + b*ld_out may lie in one row buffer (the query is read before out is written).
 * seq_len is clamped to [0, T]; ids at t >= seq_len[b] are never read; an out-of-range id at
 * t < seq_len[b] reads a zero row and raises RK_FLAG_INDEX_OOB.  Table rows 16-B aligned.
 * Envelope: H in {8,16,32}, nh in {8,16}, 1 <= T <= 256 (else RK_ERR_UNSUPPORTED).
 * Deterministic: no atomics, two launches on the same inputs are bit-equal.                     */
int rk_dien_interest(const float* query, int64_t ld_query, const float* key_table,
                     int64_t key_rows, int64_t ld_key, const int64_t* seq, int64_t ld_seq,
                     int32_t T, const int64_t* seq_len, int64_t batch, int32_t H, int32_t nh,
                     int32_t cell_type, const float* Wg, const float* bg, const float* Wc,
                     const float* bc, const float* A, const float* Vg, const float* vg,
                     const float* Vc, const float* vc, float* out, int64_t ld_out, float* att_out,
                     int64_t ld_att, void* stream);

/* rk_dien_interest with a dense history tensor: key row t of sample b at
 * keys + b * ld_keys_b + t * ld_keys_t (16-B aligned rows); rows at t >= keys_length[b] are never
 * read.  Bit-equal to rk_dien_interest on the same data.                                        */
int rk_dien_interest_dense(const float* query, int64_t ld_query, const float* keys, int64_t ld_keys_b,
                           int64_t ld_keys_t, int32_t T, const int64_t* keys_length, int64_t batch,
                           int32_t H, int32_t nh, int32_t cell_type, const float* Wg, const float* bg,
                           const float* Wc, const float* bc, const float* A, const float* Vg,
                           const float* vg, const float* Vc, const float* vc, float* out,
                           int64_t ld_out, float* att_out, int64_t ld_att, void* stream);

/* Train forward of rk_dien_interest / rk_dien_interest_dense: the same launch (out is bit-equal to
 * the eval entry points'), which also keeps what rk_dien_interest_backward needs: the extractor
 * states hs [batch, T, nh], the evolution states ss [batch, T, nh] (rows t >= seq_len[b] zero in
 * both) and the attention weights att_out [batch, T] (required here).  hs, ss 16-B aligned.
 * Same envelope.                                                                                */
int rk_dien_interest_train(const float* query, int64_t ld_query, const float* key_table,
                           int64_t key_rows, int64_t ld_key, const int64_t* seq, int64_t ld_seq,
                           int32_t T, const int64_t* seq_len, int64_t batch, int32_t H, int32_t nh,
                           int32_t cell_type, const float* Wg, const float* bg, const float* Wc,
                           const float* bc, const float* A, const float* Vg, const float* vg,
                           const float* Vc, const float* vc, float* out, int64_t ld_out,
                           float* att_out, int64_t ld_att, float* hs, float* ss, void* stream);
int rk_dien_interest_train_dense(const float* query, int64_t ld_query, const float* keys,
                                 int64_t ld_keys_b, int64_t ld_keys_t, int32_t T,
                                 const int64_t* keys_length, int64_t batch, int32_t H, int32_t nh,
                                 int32_t cell_type, const float* Wg, const float* bg, const float* Wc,
                                 const float* bc, const float* A, const float* Vg, const float* vg,
                                 const float* Vc, const float* vc, float* out, int64_t ld_out,
                                 float* att_out, int64_t ld_att, float* hs, float* ss, void* stream);

/* Request-level scoring: rk_dien_interest cut in two, for a ranking request of one history and many
 * candidates.  The interest extractor (the GRU over the history) does not read the query, so it
 * runs once per request; attention and the AGRU / AUGRU evolution run once per candidate.
 * Inference only.  Same envelope, validation and determinism as rk_dien_interest.
 *
 * rk_dien_extract: for each of `requests` histories (key_table, seq [requests, ld_seq], seq_len
 *   [requests], as rk_dien_interest takes them) writes the extractor states hs [requests, T, nh]
 *   (contiguous, 16-B aligned), rows t >= seq_len[r] zero: bit-equal to the hs of
 *   rk_dien_interest_train on the same histories.  ids at t >= seq_len[r] are never read; an
 *   out-of-range id reads a zero row and raises RK_FLAG_INDEX_OOB.  requests == 0: RK_OK, no launch.
 * rk_dien_extract_dense: the same over keys (row t of request r at keys + r*ld_keys_b + t*ld_keys_t).
 * hs is valid only for the weights Wg, bg, Wc, bc it was computed with.                           */
int rk_dien_extract(const float* key_table, int64_t key_rows, int64_t ld_key, const int64_t* seq,
                    int64_t ld_seq, int32_t T, const int64_t* seq_len, int64_t requests, int32_t H,
                    int32_t nh, const float* Wg, const float* bg, const float* Wc, const float* bc,
                    float* hs, void* stream);
int rk_dien_extract_dense(const float* keys, int64_t ld_keys_b, int64_t ld_keys_t, int32_t T,
                          const int64_t* keys_length, int64_t requests, int32_t H, int32_t nh,
                          const float* Wg, const float* bg, const float* Wc, const float* bc,
                          float* hs, void* stream);

/* rk_dien_evolve: candidate b (query row at query + b*ld_query) belongs to request
 *   r = request_index[b] (any order; a request may have no candidate or many) and gets the
 *   attention of hs[r] (rk_dien_extract's, with its seq_len [requests]) against A query[b], the
 *   masked softmax and the AGRU / AUGRU evolution: out[b, 0:nh] at out + b*ld_out and, when
 *   att_out != NULL, att_out[b, 0:T], both bit-equal to rk_dien_interest on candidate b with the
 *   history of request r.  Rows of hs at t >= seq_len[r] are never read.  A request_index outside
 *   [0, requests) is scored as an empty history (zero state, uniform attention) and raises
 *   RK_FLAG_INDEX_OOB.  query and out may lie in one row buffer.  batch == 0 or requests == 0:
 *   RK_OK, no launch, nothing written.                                                            */
int rk_dien_evolve(const float* query, int64_t ld_query, const float* hs, int64_t requests, int32_t T,
                   const int64_t* seq_len, const int64_t* request_index, int64_t batch, int32_t H,
                   int32_t nh, int32_t cell_type, const float* A, const float* Vg, const float* vg,
                   const float* Vc, const float* vc, float* out, int64_t ld_out, float* att_out,
                   int64_t ld_att, void* stream);

/* rk_dien_forward: the whole DIEN eval forward in one launch.  The row [0, width) of sample b is
 *   gathered by `row_segs` (rk_concat_gather's semantics: the last covering segment wins, an
 *   out-of-range id reads zero and raises RK_FLAG_INDEX_OOB); its columns [q_col, q_col + H) are the
 *   query of rk_dien_interest over key_table[seq[b, 0:seq_len[b]]], whose final state goes to columns
 *   [state_col, state_col + nh) (whatever a segment puts there is overwritten; the two ranges must
 *   not overlap); then `layers` (packed by rk_mlp_pack_weight) and the output layer + sigmoid of
 *   `head` (head_w / head_b / head_logit / head_prob) run over the row, which never leaves LDS.
 *   att_out (optional): the attention weights [batch, 0:T] at att_out + b*ld_att.
 *   prob, logit and att_out are bit-equal to rk_concat_gather + rk_dien_interest + rk_mlp_forward.
 * Envelope: H in {8,16,32}, nh = 8, nseg <= 32, width in (64, 128] with hidden units
 *   [512, 256, 128], history rows 16-B aligned, and an LDS need (16 samples' histories beside the
 *   row buffers, growing with T * max(H, nh)) within the CU's 160 KiB; anything else returns
 *   RK_ERR_UNSUPPORTED before any launch (the three launches compute the same).
 * Validates before launching, allocates nothing, does not synchronise, capturable.  batch == 0:
 *   RK_OK, no launch.                                                                            */
int rk_dien_forward(const rk_segment* row_segs, int32_t nseg, int32_t width, int32_t q_col,
                    int32_t state_col, const float* key_table, int64_t key_rows, int64_t ld_key,
                    const int64_t* seq, int64_t ld_seq, int32_t T, const int64_t* seq_len,
                    int64_t batch, int32_t H, int32_t nh, int32_t cell_type, const float* Wg,
                    const float* bg, const float* Wc, const float* bc, const float* A,
                    const float* Vg, const float* vg, const float* Vc, const float* vc,
                    const rk_mlp_layer* layers, int32_t nlayers, const rk_epilogue* head,
                    float* att_out, int64_t ld_att, void* stream);
/* A prepared rk_dien_forward, as rk_din_forward_plan: the same arguments, validated once, launched
 * later by rk_dien_plan_launch on any stream at the cost of one kernel launch.  A plan binds the
 * pointers it was made with: keep every buffer alive, and make a new plan after the weights move
 * or their packed images are rebuilt.                                                           */
int rk_dien_forward_plan(const rk_segment* row_segs, int32_t nseg, int32_t width, int32_t q_col,
                         int32_t state_col, const float* key_table, int64_t key_rows,
                         int64_t ld_key, const int64_t* seq, int64_t ld_seq, int32_t T,
                         const int64_t* seq_len, int64_t batch, int32_t H, int32_t nh,
                         int32_t cell_type, const float* Wg, const float* bg, const float* Wc,
                         const float* bc, const float* A, const float* Vg, const float* vg,
                         const float* Vc, const float* vc, const rk_mlp_layer* layers,
                         int32_t nlayers, const rk_epilogue* head, float* att_out, int64_t ld_att,
                         void** plan);
int rk_dien_plan_launch(const void* plan, void* stream);
void rk_dien_plan_destroy(void* plan);

/* Backward of the interest recurrence (backprop through time, t = seq_len-1 ... 0) given
 * d_out[b, 0:nh] = dL/d(out) at d_out + b*ld_dout and the forward's inputs, hs, ss and att:
 *   dquery[b, 0:H] at dquery + b*ld_dquery (added to when accumulate_dquery; d_out and dquery may
 *   lie in one row-gradient buffer), dkeys [batch, T, H] contiguous = dL/d(key row t of sample b)
 *   (rows t >= seq_len[b] exact zeros; every row written), and the nine weight gradients, shaped
 *   like the weights (overwritten).  A sample with seq_len 0 has zero gradients.
 * Key source: seq != NULL: keys = the table [key_rows, ld_key], ids seq [batch, ld_seq] (an
 * out-of-range id at t < seq_len reads the zero row, as in the forward); seq == NULL: keys = the
 * dense history, row t of sample b at keys + b*ld_keys_b + t*ld_key.
 * seq_masked (NULL, or [batch, T] with seq): the ids with 0 at t >= seq_len[b], the index list
 * for rk_embedding_backward of dkeys into the table's gradient.
 * One chain launch (one 16-lane row per sample) that also writes the per-step pre-activation
 * gradients and operand rows into the workspace; dkeys is two rk_gemm products and the weight
 * gradients are rk_gemm_wgrad products over those rows: no float atomics, deterministic.
 * workspace: rk_dien_interest_backward_workspace_floats(batch, T, H, nh) floats, 16-B aligned.
 * Envelope and alignment as the forward (else RK_ERR_UNSUPPORTED).                              */
int64_t rk_dien_interest_backward_workspace_floats(int64_t batch, int32_t T, int32_t H, int32_t nh);
int rk_dien_interest_backward(const float* query, int64_t ld_query, const float* keys, int64_t key_rows,
                              int64_t ld_key, const int64_t* seq, int64_t ld_seq, int64_t ld_keys_b,
                              int32_t T, const int64_t* seq_len, int64_t batch, int32_t H, int32_t nh,
                              int32_t cell_type, const float* Wg, const float* bg, const float* Wc,
                              const float* bc, const float* A, const float* Vg, const float* vg,
                              const float* Vc, const float* vc, const float* hs, const float* ss,
                              const float* att, int64_t ld_att, const float* d_out, int64_t ld_dout,
                              float* dquery, int64_t ld_dquery, int32_t accumulate_dquery, float* dkeys,
                              float* dWg, float* dbg, float* dWc, float* dbc, float* dA, float* dVg,
                              float* dvg, float* dVc, float* dvc, int64_t* seq_masked, float* workspace,
                              int64_t workspace_floats, void* stream);

/* rk_dien_interest_backward with a second source of dL/dh_t and an accumulating dkeys, for a loss
 * that reads the extractor states themselves (rk_dien_aux_loss):
 *   d_hs (NULL, or [batch, T, nh] contiguous): added to dL/dh_t inside the extractor's backward
 *   chain for t < seq_len[b]; rows t >= seq_len[b] are never read.
 *   accumulate_dkeys: the history-row gradients are added to dkeys (every row of which the caller
 *   has written, e.g. rk_dien_aux_loss_backward) instead of overwriting it.
 * With d_hs == NULL and accumulate_dkeys == 0 this is rk_dien_interest_backward, bit for bit (that
 * entry point forwards here).  Same workspace query.                                            */
int rk_dien_interest_backward_aux(const float* query, int64_t ld_query, const float* keys, int64_t key_rows,
                                  int64_t ld_key, const int64_t* seq, int64_t ld_seq, int64_t ld_keys_b,
                                  int32_t T, const int64_t* seq_len, int64_t batch, int32_t H, int32_t nh,
                                  int32_t cell_type, const float* Wg, const float* bg, const float* Wc,
                                  const float* bc, const float* A, const float* Vg, const float* vg,
                                  const float* Vc, const float* vc, const float* hs, const float* ss,
                                  const float* att, int64_t ld_att, const float* d_out, int64_t ld_dout,
                                  float* dquery, int64_t ld_dquery, int32_t accumulate_dquery, float* dkeys,
                                  float* dWg, float* dbg, float* dWc, float* dbc, float* dA, float* dVg,
                                  float* dvg, float* dVc, float* dvc, int64_t* seq_masked, const float* d_hs,
                                  int32_t accumulate_dkeys, float* workspace, int64_t workspace_floats,
                                  void* stream);

/* DIEN auxiliary loss (DIEN/dien.py:256-300, with the paper's sign): every extractor state h_t is
 * scored against the next behaviour e_{t+1} and against T_neg sampled negatives n_{t,k}:
 *   g_t = W_aux h_t (W_aux [H, nh] row-major);  pos_t = g_t . e_{t+1};  neg_{t,k} = g_t . n_{t,k}
 *   per_sample[b] = - sum_{t < seq_len[b]-1} [ logsig(pos_t) + sum_k logsig(-neg_{t,k}) ]
 *   mean[0]       = (1 / batch) sum_b per_sample[b]
 * with logsig(x) = min(x, 0) - log1p(exp(-|x|)).  A sample with seq_len <= 1 (or T == 1) gives 0.
 * hs [batch, T, nh] contiguous: the states rk_dien_interest_train keeps.  History rows as
 * rk_dien_interest takes them (key_table, seq [batch, ld_seq]); the negatives are rows of the same
 * table, ids neg_seq [batch, ld_neg_seq], entry t * T_neg + k pairs with h_t (ld_neg_seq >=
 * (T-1) T_neg; neg_seq may be NULL when T == 1).  seq_len is clamped to [0, T]; ids of masked
 * steps (history t+1 >= seq_len, negatives of t >= seq_len-1) are never read; an out-of-range id at
 * a live step reads a zero row and raises RK_FLAG_INDEX_OOB.  hs and table rows 16-B aligned.
 * Envelope: H in {8,16,32}, nh in {8,16}, 1 <= T <= 256, 1 <= T_neg <= 8 (else RK_ERR_UNSUPPORTED,
 * before any launch).  One wave per sample, H/4 lanes per (b, t) item; fixed-order sums, no atomics:
 * two launches on the same inputs are bit-equal.                                                 */
int rk_dien_aux_loss(const float* hs, const float* key_table, int64_t key_rows, int64_t ld_key,
                     const int64_t* seq, int64_t ld_seq, const int64_t* neg_seq, int64_t ld_neg_seq,
                     int32_t T, int32_t T_neg, const int64_t* seq_len, int64_t batch, int32_t H, int32_t nh,
                     const float* W_aux, float* per_sample, float* mean, void* stream);

/* rk_dien_aux_loss over dense tensors: history row t of sample b at keys + b*ld_keys_b + t*ld_keys_t,
 * negative row i (= t * T_neg + k) at neg + b*ld_neg_b + i*ld_neg_r (16-B aligned rows; rows of
 * masked steps are never read).  Bit-equal to rk_dien_aux_loss on the same data.                 */
int rk_dien_aux_loss_dense(const float* hs, const float* keys, int64_t ld_keys_b, int64_t ld_keys_t,
                           const float* neg, int64_t ld_neg_b, int64_t ld_neg_r, int32_t T, int32_t T_neg,
                           const int64_t* seq_len, int64_t batch, int32_t H, int32_t nh, const float* W_aux,
                           float* per_sample, float* mean, void* stream);

/* Backward of the auxiliary loss given d_loss[0] = dL/d(mean), read on the device (the call is
 * graph-capturable); the dots are recomputed.  With k = d_loss[0] / batch, cpos = -k sig(-pos_t),
 * cneg_k = k sig(neg_{t,k}), dg_t = cpos e_{t+1} + sum_k cneg_k n_{t,k}:
 *   d_hs  [batch, T, nh]          = W_aux^T dg_t        (rows t >= seq_len-1 exact zeros)
 *   dkeys [batch, T, H]           row t+1 = cpos g_t    (row 0 and rows >= seq_len exact zeros)
 *   dneg  [batch, (T-1) T_neg, H] row t*T_neg+k = cneg_k g_t (exact zeros for t >= seq_len-1)
 *   dW_aux [H, nh]                = sum_{b,t} dg_t h_t^T
 * all contiguous, 16-B aligned, every element written.  Sources: seq != NULL: keys = the table,
 * ids seq / neg_seq as in the forward, neg ignored; neg_masked (NULL or [batch, (T-1) T_neg])
 * receives the negative ids with 0 at masked steps and seq_masked (NULL or [batch, T]) the history
 * ids with 0 wherever dkeys is zero (t == 0, t >= seq_len), the index lists for
 * rk_embedding_backward of dneg and of dkeys.  seq == NULL: keys / neg dense as in
 * rk_dien_aux_loss_dense (ld_key = the history's row stride), neg_seq and both masked lists NULL.  One item kernel writes dg rows to the workspace; d_hs is
 * one rk_gemm and dW_aux one rk_gemm_wgrad over them: fixed-order sums, no float atomics.
 * workspace: rk_dien_aux_loss_backward_workspace_floats(batch, T, H, nh) floats, 16-B aligned.   */
int64_t rk_dien_aux_loss_backward_workspace_floats(int64_t batch, int32_t T, int32_t H, int32_t nh);
int rk_dien_aux_loss_backward(const float* hs, const float* keys, int64_t key_rows, int64_t ld_key,
                              const int64_t* seq, int64_t ld_seq, int64_t ld_keys_b, const float* neg,
                              int64_t ld_neg_b, int64_t ld_neg_r, const int64_t* neg_seq, int64_t ld_neg_seq,
                              int32_t T, int32_t T_neg, const int64_t* seq_len, int64_t batch, int32_t H,
                              int32_t nh, const float* W_aux, const float* d_loss, float* d_hs, float* dkeys,
                              float* dneg, int64_t* seq_masked, int64_t* neg_masked, float* dW_aux,
                              float* workspace, int64_t workspace_floats, void* stream);

/* Dice (din.py:26-36) in eval: p = sigmoid(x * bn_scale + bn_shift) with the BatchNorm folded
 * by rk_bn_fold, y = alpha * (1 - p) * x + p * x;  x, y: [rows, n].                          */
int rk_dice_forward(const float* x, int64_t ldx, int64_t rows, int32_t n, const float* bn_scale,
                    const float* bn_shift, const float* alpha, float* y, int64_t ldy, void* stream);

/* out_scalar = scale * mean_r ||x[r, col0:col0+ncols]||_2, deterministic two-stage sum;
 * workspace: RK_L2_WORKSPACE floats of device scratch.                                   */
#define RK_L2_WORKSPACE 512
int rk_row_l2norm_mean(const float* x, int64_t ld, int64_t rows, int32_t col0, int32_t ncols,
                       float scale, float* workspace, float* out_scalar, void* stream);

/* Whole DIN eval forward (din.py:294-323) in one launch:
 *   row[b] = concat(row_segs)  (width <= 255; target query at q_col, attention written at att_col)
 *   row[b, att_col:+H] = din_attention(row[b, q_col:+H], key_table[seq[b]], seq_len[b])
 *   head outputs = fcn layers (rk_mlp_layer, packed) + head (head_w/head_b/head_logit/head_prob)
 *   l2_out = l2_scale * mean_b ||row[b, l2_col0:width]||_2 when l2_out != NULL, finished in
 *     the same launch by the last workgroup.  l2_workspace: ceil(batch/16) floats of partials
 *     followed by one uint32 counter that must be 0 before the first call (the kernel leaves it
 *     0 again; keep one workspace per stream).  H in {8, 16, 32}.                          */
int rk_din_forward(const rk_segment* row_segs, int32_t nseg, int32_t width, int32_t q_col,
                   int32_t att_col, const float* key_table, int64_t key_rows, int64_t ld_key,
                   const int64_t* seq, int64_t ld_seq, int32_t T, const int64_t* seq_len,
                   int64_t batch, int32_t H, const float* w1, const float* b1, const float* w2,
                   const float* b2, const float* w3, const float* b3, int32_t use_softmax,
                   const rk_mlp_layer* layers, int32_t nlayers, const rk_epilogue* head,
                   int32_t l2_col0, float l2_scale, float* l2_workspace, float* l2_out,
                   const float* att_image, void* stream);

/* att_image (optional, NULL = split in the kernel from w1..w3): the attention weights pre-split
 * into the kernel's LDS layout by rk_din_pack_attention (rk_din_attention_image_floats(H)
 * floats, 16-B aligned), so the launch stages them with one round of coalesced copies.  The
 * layout splits W1 = [W1a | W1b | W1c | W1d] over [q, k, q-k, q*k] (din.py:56-64): WK = W1b - W1c,
 * WQK = W1d, WQ = W1a + W1c, then W2, b1, b2, w3 (b3 is read from its pointer).              */
int64_t rk_din_attention_image_floats(int32_t H);
int rk_din_pack_attention(const float* w1, const float* b1, const float* w2, const float* b2,
                          const float* w3, int32_t H, float* image, void* stream);

/* rk_din_forward with phase B's epilogue-parameter image packed by rk_mlp_pack_epilogue from the
 * same layer stack (NULL: resolved per column at launch, as rk_din_forward): the kernel copies it
 * into LDS by LDS-DMA after the attention phase.  Ignored when phase B does not run on the
 * compiled [512, 256, 128] plan.  Same outputs, bit for bit.                                  */
int rk_din_forward_ex(const rk_segment* row_segs, int32_t nseg, int32_t width, int32_t q_col,
                      int32_t att_col, const float* key_table, int64_t key_rows, int64_t ld_key,
                      const int64_t* seq, int64_t ld_seq, int32_t T, const int64_t* seq_len,
                      int64_t batch, int32_t H, const float* w1, const float* b1, const float* w2,
                      const float* b2, const float* w3, const float* b3, int32_t use_softmax,
                      const rk_mlp_layer* layers, int32_t nlayers, const rk_epilogue* head,
                      int32_t l2_col0, float l2_scale, float* l2_workspace, float* l2_out,
                      const float* att_image, const float* epi_image, void* stream);

/* A prepared rk_din_forward: the same arguments, validated once, launched later by
 * rk_din_plan_launch on any stream at the cost of one kernel launch — the one-kernel analogue of
 * a captured hipGraph without the graph's per-replay launch gap (~9 us on this forward).  Like a
 * graph, a plan binds the pointers it was made with: keep every buffer alive, and make a new plan
 * after the weights move or their packed images are rebuilt.                                  */
int rk_din_forward_plan(const rk_segment* row_segs, int32_t nseg, int32_t width, int32_t q_col,
                        int32_t att_col, const float* key_table, int64_t key_rows, int64_t ld_key,
                        const int64_t* seq, int64_t ld_seq, int32_t T, const int64_t* seq_len,
                        int64_t batch, int32_t H, const float* w1, const float* b1, const float* w2,
                        const float* b2, const float* w3, const float* b3, int32_t use_softmax,
                        const rk_mlp_layer* layers, int32_t nlayers, const rk_epilogue* head,
                        int32_t l2_col0, float l2_scale, float* l2_workspace, float* l2_out,
                        const float* att_image, void** plan);
int rk_din_plan_launch(const void* plan, void* stream);
void rk_din_plan_destroy(void* plan);
/* Binds the plan's phase-B epilogue-parameter image, packed by rk_mlp_pack_epilogue from the same
 * layer stack (NULL unbinds): its launches then copy it into LDS by LDS-DMA after the attention
 * phase instead of resolving every column's bias / BatchNorm / Dice parameters at launch.
 * RK_ERR_UNSUPPORTED for a plan without a streamed phase B.                                     */
int rk_din_plan_set_epilogue_image(void* plan, const float* image);

int rk_afm_forward(const rk_segment* fields, int32_t num_fields, int32_t dim, int64_t batch,
                   const float* dense, int64_t ld_dense, int32_t num_dense,
                   const float* dense_w, const float* dense_b, const float* att_w,
                   const float* att_b, int32_t att_factor, const float* att_h,
                   const float* att_hb, const float* p_w, const float* p_b, float* logit,
                   float* prob, void* stream);

int rk_bst_attention(const float* qkv, int64_t ld_qkv, int64_t batch, int32_t T,
                     int32_t d_model, int32_t heads, const int64_t* seq_len, float* ctx,
                     int64_t ld_ctx, void* stream);
/* key_padding_mask: [batch, ld_mask] bytes, nonzero = masked key (torch bool); NULL = none.
 * A row with every key masked gives NaN context, as torch's softmax over all -inf.          */
int rk_bst_attention_masked(const float* qkv, int64_t ld_qkv, int64_t batch, int32_t T,
                            int32_t d_model, int32_t heads, const uint8_t* key_padding_mask,
                            int64_t ld_mask, float* ctx, int64_t ld_ctx, void* stream);

/* The whole BSTModel eval forward at the reference script's d_model 16 (bst.py:192, 216-247) in one
 * launch: the DNN row [dense | category embeddings] gathered by `row_segs` over columns
 * [0, width), every transformer block and the pooling (as rk_bst_forward_blocks at d_model 16)
 * written to columns [width, width + 16), then `layers` (packed by rk_mlp_pack_weight, BatchNorm
 * folded, LeakyReLU) and the output layer + sigmoid of `head` (head_w/head_b/head_logit/head_prob).
 * Envelope: heads 1/2/4/8, 1 <= T <= 64, nblocks <= 4, nseg <= 8, width + 16 in (64, 128] with
 * hidden units [512, 256, 128] (else RK_ERR_UNSUPPORTED: rk_concat_gather +
 * rk_bst_forward_blocks + rk_mlp_forward compute the same).                                  */
int rk_bst_small_forward(const rk_segment* row_segs, int32_t nseg, int32_t width, const float* table,
                         int64_t table_rows, int64_t ld_table, const int64_t* seq, int64_t ld_seq,
                         int32_t T, const int64_t* seq_len, int64_t batch, int32_t heads,
                         int32_t nblocks, const float* const* block_params,
                         const float* block_scalars, int32_t pool_mean, const rk_mlp_layer* layers,
                         int32_t nlayers, const rk_epilogue* head, void* stream);

/* Every transformer block of BSTModel.forward plus the pooling (bst.py:66-91, 224-241) in one
 * launch, one workgroup per sample, activations kept in LDS:
 *   x = table[seq[b, :T]];  for each block i: x = block_i(x)  (mask keys >= seq_len[b])
 *   pool_out[b, 0:128] = sum_t x[t]  (/ seq_len[b] when pool_mean)
 * block_params: host array of 17 device pointers per block, in this order:
 *   pos[max_len,128], wq, bq, wk, bk, wv, bv, wo, bo, w1 (ffn.0), b1, w2 (ffn.3), b2,
 *   ln1_gamma, ln1_beta, ln2_gamma, ln2_beta   (nn.Linear [out,in] row-major, 16-B aligned)
 * block_scalars: host array of 3 floats per block: ln1_eps, ln2_eps, leaky slope.
 * Envelope: d_model 128, heads 4, 1 <= T <= 64, nblocks <= 4 (else RK_ERR_UNSUPPORTED).
 * Replaces the rk_linear x5 + rk_bst_attention sequence of one block.                     */
int rk_bst_forward_blocks(const float* table, int64_t table_rows, int64_t ld_table,
                          const int64_t* seq, int64_t ld_seq, int32_t T, const int64_t* seq_len,
                          int64_t batch, int32_t d_model, int32_t heads, int32_t nblocks,
                          const float* const* block_params, const float* block_scalars,
                          float* pool_out, int64_t ld_pool, int32_t pool_mean, void* stream);
/* rk_bst_forward_blocks (d_model 128 only) with the six projection weights of every block (wq, wk,
 * wv, wo, w1, w2) in rk_bst_pack_block_weight's layout; same outputs, bit for bit.            */
int rk_bst_forward_blocks_packed(const float* table, int64_t table_rows, int64_t ld_table,
                                 const int64_t* seq, int64_t ld_seq, int32_t T,
                                 const int64_t* seq_len, int64_t batch, int32_t d_model,
                                 int32_t heads, int32_t nblocks, const float* const* block_params,
                                 const float* block_scalars, float* pool_out, int64_t ld_pool,
                                 int32_t pool_mean, void* stream);
/* A [128, 128] projection weight (nn.Linear [out, in], contiguous) in the order the block kernel's
 * 32x32x2 MFMA lanes load it: float 4096 j + 1024 g + 256 c + 4 l + e of `out` (16384 floats) is
 * W[32 j + l % 32][32 g + 8 c + 4 (l / 32) + e] — each wave load one contiguous 1 KiB.  Not in place. */
int rk_bst_pack_block_weight(const float* w, float* out, void* stream);

/* ---- dense layers ---- */
int rk_linear(const float* x, int64_t ldx, const float* x_periodic, int32_t x_period,
              const float* w, int64_t ldw, int64_t M, int32_t N, int32_t K,
              const rk_epilogue* ep, float* y, int64_t ldy, void* stream);

/* Packed layout of a fused-MLP weight: pad64(n) x pad64(k) floats, zero filled (rows and K
 * padded to 64 so the kernel's loads are unconditional aligned float4s), fragment-major: the
 * 16-column x 16-k block (t, c) is 256 contiguous floats in the order the MFMA lanes load it
 * (float i of the block = W[16t + ((i>>2)&15)][16c + 4((i>>2)>>4) + (i&3)]).  Pack once at load
 * time; rows/cols of rk_mlp_packed_size give the size and ldw = cols.                       */
int rk_mlp_packed_size(int32_t n, int32_t k, int64_t* rows, int64_t* cols);
int rk_mlp_pack_weight(const float* w, int64_t ldw, int32_t n, int32_t k, float* out, void* stream);

/* The per-column epilogue parameters of a layer stack with a compiled streamed plan (hidden units
 * [512, 256, 128] over an input of <= 256, or [256, 128] over 512), resolved and laid out as the
 * streamed tail's LDS image ([column][8] floats: bias, pre scale/shift, Dice scale/shift, slope,
 * post scale/shift).  rk_mlp_epilogue_image_floats: its size in floats (0: no compiled plan).    */
int rk_mlp_epilogue_image_floats(const rk_mlp_layer* layers, int32_t nlayers, int32_t K0);
int rk_mlp_pack_epilogue(const rk_mlp_layer* layers, int32_t nlayers, int32_t K0, float* out, void* stream);

/* Whole MLP tail in one launch: layers[0..nlayers) on x [M, K0] (K0 <= 1024, widths <= 512;
 * every layers[l].w packed by rk_mlp_pack_weight, ldw = pad64(K)), then the head of `head`
 * (head_w/head_b/head_partial/fm combine/head_logit/head_prob/head_aux) when head->head_w is
 * set, else the last activation is written to y.                                          */
int rk_mlp_forward(const float* x, int64_t ldx, int64_t M, int32_t K0, const rk_mlp_layer* layers,
                   int32_t nlayers, const rk_epilogue* head, float* y, int64_t ldy, void* stream);

/* rk_concat_gather + rk_mlp_forward in one launch (eval, generic tail with residual layers, a head):
 * each 16-row workgroup gathers its rows' `width` columns from the segments (rk_concat_gather's
 * column map: the last covering segment wins, uncovered columns are zero, out-of-range rows are
 * zero and raise RK_FLAG_INDEX_OOB) straight into the first layer's LDS buffer.  nseg <= 16,
 * width <= 256, head->head_w required, no layer stores.  Replaces the reference's
 * torch.cat(dense, embeddings) + residual stack + output layer (deepcrossing.py:146-163).       */
int rk_mlp_forward_gather(const rk_segment* segs, int32_t nseg, int32_t width, int64_t batch,
                          const rk_mlp_layer* layers, int32_t nlayers, const rk_epilogue* head, void* stream);

/* Whole DCN eval forward in one launch (DCNModel.forward, dcn.py:161-180): gather of the row from
 * segs (out_col ascending from 0, at most 8 segments, width <= 256), num_layers cross layers
 * (weights [L, width] as rk_dcn_cross), the MLP tail as rk_mlp_forward (layers packed) and the head:
 * logit = x_L . cross_head_w + (h . head->head_w + head->head_b), prob = sigmoid(logit), written to
 * head->head_logit / head->head_prob.  cross_head_w = output_layer.weight[0, :width].           */
int rk_dcn_forward(const rk_segment* segs, int32_t nseg, int64_t batch, int32_t width, const float* cross_w,
                   const float* cross_b, int32_t num_layers, const float* cross_head_w,
                   const rk_mlp_layer* layers, int32_t nlayers, const rk_epilogue* head, void* stream);

/* One MLP layer as a 2D-tiled GEMM (64-row x 128-column tiles): y[M, n] = epilogue(x . W^T) with
 * W packed by rk_mlp_pack_weight (ldw = pad64(K)) and the element-wise part of the rk_mlp_layer
 * epilogue (bias, BatchNorm affines, activation; no residual).  For a wide first layer
 * (deepfm.py:100-112, 960 -> 512) it reads every weight 64 times per 4096 rows instead of 256. */
int rk_linear_tiled(const float* x, int64_t ldx, int64_t M, int32_t K, const rk_mlp_layer* layer,
                    float* y, int64_t ldy, void* stream);

/* The DeepFM eval front end as one 2D-tiled launch (deepfm.py:122-142 then deepfm.py:100-112 for the
 * first deep layer): for every sample b, fm1[b] = sum_f first-order weight, fm2[b] = 0.5 sum_d
 * ((sum_f e_f)^2 - sum_f e_f^2)[d], and y[b, :] = epilogue(concat_f(e_f) . W^T) with
 * e_f = row idx_f[b] of field f's packed table (rk_fm_pack_table layout, as rk_fm_gather_packed:
 * segment f = {packed table, unit-stride index, rows, dim, src_ld >= dim + 1, out_col = f * dim}).
 * A segment with idx = NULL is a dense block of packed rows (row b at src + b * src_ld, b < batch):
 * the rows ShardedDeepFM receives from a field's owner rank over the row all-to-all.
 * The layer is packed by rk_mlp_pack_weight for K = num_fields * dim (no residual).  dim a power of
 * two in [4, 256], num_fields <= 32.  The concatenated deep input is staged in LDS only.
 * Out-of-range indices read zero rows and raise RK_FLAG_INDEX_OOB.                               */
int rk_fm_linear_packed(const rk_segment* fields, int32_t num_fields, int32_t dim, int64_t batch,
                        const rk_mlp_layer* layer, float* y, int64_t ldy, float* fm1, float* fm2,
                        void* stream);

/* The whole DeepFM eval forward in one launch (DeepFM.forward, deepfm.py:121-151): fields as for
 * rk_fm_linear_packed (packed tables with unit-stride indices, or dense blocks of packed rows),
 * layers = the three deep layers (Linear + BatchNorm folded + ReLU, deepfm.py:100-112), head =
 * deep_output_layer (head_w, head_b) with final_layer (final_w, final_b) and the outputs
 * head_logit / head_prob / head_aux (the deep logit); fm1 / fm2 [batch] are written (its own
 * fm1 / fm2 fields are ignored).  Compiled plan: 960 -> 512 -> 256 -> 128 (configs[1]: 30 fields
 * x 32); other shapes return RK_ERR_UNSUPPORTED (use rk_fm_linear_packed + rk_mlp_forward). */
int rk_deepfm_forward(const rk_segment* fields, int32_t num_fields, int32_t dim, int64_t batch,
                      const rk_mlp_layer* layers, int32_t nlayers, const rk_epilogue* head, float* fm1,
                      float* fm2, void* stream);

/* ---- xDeepFM: the Compressed Interaction Network (Lian et al. 2018, eq. 6-8, direct form) ---- */
/* One CIN layer's weight W [n, k] (nn.Conv1d(k, n, 1).weight, k = H_prev * num_fields, row stride
 * ldw) as the image rk_cin_forward streams: pad16(n) * pad16(k) floats, zero padded, in the load
 * order of v_mfma_f32_16x16x4_f32's A operand:
 *   out[((mt * pad16(k)/16 + ks) * 64 + lane) * 4 + e] = W[16 mt + lane % 16][16 ks + 4 e + lane / 16].
 * A layout pass run once per weight version (the host layer caches it).  out 16-B aligned.      */
int rk_cin_pack_weight(const float* w, int64_t ldw, int32_t n, int32_t k, float* out, void* stream);

/* The xDeepFM front end in one launch.  second_order: num_fields segments of `dim` columns, all
 * tables or all dense, rows 16-B aligned (src_ld % 4 == 0), out_col % 4 == 0 = the field's column
 * in deep_in; x0[b, i, :] = the row of field i.  For k = 1..num_layers, with H_0 = num_fields:
 *   x^k[b, n, d] = act( sum_{h, i} W_k[n, h * num_fields + i] * x^{k-1}[b, h, d] * x0[b, i, d] + biases[k][n] )
 * (weights[k]: the rk_cin_pack_weight image of W_k [layer_sizes[k], layer_sizes[k-1] * num_fields];
 * biases[k] may be NULL; activation RK_ACT_NONE or RK_ACT_RELU), then
 *   pooled[b, off_k + n] = sum_d x^k[b, n, d]   (off_k = layer_sizes[0] + .. + layer_sizes[k-1])
 *   cin_logit[b] = pooled[b, :] . out_w + out_b[0].
 * Outputs, each may be NULL: deep_in [batch, ld_deep] (the gathered rows, 16-B aligned, ld_deep % 4
 * == 0), fm1 [batch] = the sum over fields, in order, of first_order's one-column segments (tables
 * or dense as second_order; first_order may be NULL when fm1 is), pooled [batch, ld_pooled],
 * cin_logit [batch] (needs out_w, out_b).  The feature maps stay in LDS; sums run in a fixed order
 * (no atomics), so two launches give the same bits.
 * Envelope: 2 <= num_fields <= 32, dim in {4, 8, 16, 32, 64}, 1 <= num_layers <= 4,
 * 1 <= layer_sizes[k] <= 256 (else RK_ERR_UNSUPPORTED); NULL or shape errors: RK_ERR_INVALID before
 * any launch; batch == 0: RK_OK, no launch.  Out-of-range ids read zero rows and raise
 * RK_FLAG_INDEX_OOB.                                                                            */
int rk_cin_forward(const rk_segment* second_order, const rk_segment* first_order, int32_t num_fields,
                   int32_t dim, int64_t batch, const float* const* weights, const float* const* biases,
                   const int32_t* layer_sizes, int32_t num_layers, int32_t activation,
                   const float* out_w, const float* out_b, float* deep_in, int64_t ld_deep, float* fm1,
                   float* pooled, int64_t ld_pooled, float* cin_logit, void* stream);

/* ---- FiBiNET: SENET field attention and the bilinear interaction (Huang et al., RecSys 2019) ---- */
#define RK_FIBINET_ALL 0         /* one D x D matrix for every pair                          */
#define RK_FIBINET_EACH 1        /* one per left field i < num_fields - 1                    */
#define RK_FIBINET_INTERACTION 2 /* one per pair (i, j), i < j, pairs in lexicographic order */

/* SENET and both bilinear layers in one launch.  second_order: num_fields segments of `dim` columns,
 * all tables or all dense, rows 16-B aligned (src_ld % 4 == 0; out_col is not read);
 * e[b, i, :] = the row of field i.  With m = num_fields, r = reduced, pair p = (i, j), i < j:
 *   z[b, i] = mean_d e[b, i, d],  a[b, :] = relu(W2 relu(W1 z[b, :])),  v[b, i, :] = a[b, i] e[b, i, :]
 *   c[b, p * dim + d]                 = (We e[b, i, :])[d] * e[b, j, d]
 *   c[b, (m (m-1)/2 + p) * dim + d]   = (Wv v[b, i, :])[d] * v[b, j, d]
 * senet_w1 [r, m] and senet_w2 [m, r] row-major (nn.Linear's weights, no bias); bilinear_e and
 * bilinear_v: the stacked [nmat, dim, dim] row-major nn.Linear weights (W x = x . W^T), 16-B aligned,
 * nmat = 1 / m - 1 / m (m-1)/2 and We = matrix 0 / i / p by bilinear_type.
 * Outputs: c [batch, ldc] (required, ldc >= m (m-1) dim); linear [batch] = the sum over fields, in
 * order, of first_order's one-column segments (may be NULL, first_order then too); attention
 * [batch, ld_attention] = a (may be NULL).  Rows, products and attention stay in LDS; fp32 on the
 * VALU, every sum in a fixed order (no atomics): two launches give the same bits.
 * Envelope: 2 <= num_fields <= 32, dim a multiple of 4 in [4, 64], reduced <= 32 (else
 * RK_ERR_UNSUPPORTED); NULL or shape errors and batch < 0: RK_ERR_INVALID; both before any launch.
 * batch == 0: RK_OK, no launch.  Out-of-range ids read zero rows and raise RK_FLAG_INDEX_OOB.     */
int rk_fibinet_interaction(const rk_segment* second_order, const rk_segment* first_order, int32_t num_fields,
                           int32_t dim, int64_t batch, const float* senet_w1, const float* senet_w2,
                           int32_t reduced, const float* bilinear_e, const float* bilinear_v,
                           int32_t bilinear_type, float* c, int64_t ldc, float* linear, float* attention,
                           int64_t ld_attention, void* stream);

/* The whole FiBiNET eval forward in one launch: per 16-row workgroup the row gather,
 * the first-order sum, rk_fibinet_interaction's c written straight into the MLP's LDS input row, the
 * deep layers as rk_mlp_forward (layers packed by rk_mlp_pack_weight for K0 = m (m-1) dim; Linear,
 * folded BatchNorm, activation), then
 *   deep = h . head_w + head_b[0],  total = final_w[0] * linear + final_w[1] * deep + final_b[0],
 *   prob = sigmoid(total)
 * into linear / deep_logit / total_logit / prob [batch] (each may be NULL, not all).  first_order
 * is required.  Envelope: rk_fibinet_interaction's, with m (m-1) dim <= 1024, 1..8 layers of n <= 512
 * without residual or store, and the two activation buffers, the rows and the products within
 * 160 KiB of LDS (else RK_ERR_UNSUPPORTED: rk_fibinet_interaction + rk_mlp_forward compute the same).
 * Errors, batch == 0 and out-of-range ids as rk_fibinet_interaction.                              */
int rk_fibinet_forward(const rk_segment* second_order, const rk_segment* first_order, int32_t num_fields,
                       int32_t dim, int64_t batch, const float* senet_w1, const float* senet_w2,
                       int32_t reduced, const float* bilinear_e, const float* bilinear_v,
                       int32_t bilinear_type, const rk_mlp_layer* layers, int32_t nlayers, const float* head_w,
                       const float* head_b, const float* final_w, const float* final_b, float* linear,
                       float* deep_logit, float* total_logit, float* prob, void* stream);

/* ---- MMoE: multi-gate mixture of experts (Ma et al., KDD 2018), eval forward ---- */
/* One Linear (+ ReLU) of an expert or a tower: w = the rk_mlp_pack_weight image of W [n, K] (K = the
 * previous layer's n, or the row width / the experts' output width for a first layer), bias [n] or
 * NULL, act RK_ACT_NONE or RK_ACT_RELU.                                                          */
typedef struct rk_mmoe_layer {
  const float* w;
  const float* bias;
  int32_t n;
  int32_t act;
} rk_mmoe_layer;

/* The whole MMoE eval forward in one launch.  Per row b, with x = the `width` columns gathered from
 * segs (rk_mlp_forward_gather's column map; out-of-range ids read zero rows and raise
 * RK_FLAG_INDEX_OOB):
 *   f_e = experts[e](x)                       experts[e * expert_depth + l], l = 0 .. expert_depth - 1;
 *                                             every expert ends H wide
 *   g_k = softmax_e(x . gate_w[k E + e] + gate_b[k E + e])    gate_w: the rk_mlp_pack_weight image of the
 *                                             num_tasks gate weights stacked to [num_tasks * num_experts,
 *                                             width]; gate_b [num_tasks * num_experts] or NULL
 *   m_k = sum_e g_k[e] f_e                    e ascending, FP32, no atomics: two launches give the same bits
 *   logit_k = towers[k](m_k) . head_w[k] + head_b[k][0]      towers[k * tower_depth + l]; head_w[k] [last width]
 *   prob_k = sigmoid(logit_k)
 * Outputs, each may be NULL: logits, probs [batch, num_tasks]; mixed [batch, num_tasks, H] (m_k);
 * gate_probs [batch, num_tasks, num_experts] (g_k), all contiguous.  head_w = head_b = NULL (then towers
 * = NULL, tower_depth = 0, logits = probs = NULL) stops after the mix.  [batch, E, H] is never formed.
 * Envelope: nseg <= 16 segments of at most 255 columns each, width <= 256, num_experts <= 16, num_tasks <= 8, num_tasks * num_experts <= 64,
 * 1 <= expert_depth <= 3, 0 <= tower_depth <= 3, every n <= 512, activations none / ReLU (else
 * RK_ERR_UNSUPPORTED); NULL or shape errors and batch < 0: RK_ERR_INVALID; both before any launch.
 * batch == 0: RK_OK, no launch.                                                                   */
int rk_mmoe_forward(const rk_segment* segs, int32_t nseg, int32_t width, int64_t batch,
                    const rk_mmoe_layer* experts, int32_t num_experts, int32_t expert_depth,
                    const float* gate_w, const float* gate_b, int32_t num_tasks, const rk_mmoe_layer* towers,
                    int32_t tower_depth, const float* const* head_w, const float* const* head_b, float* logits,
                    float* probs, float* mixed, float* gate_probs, void* stream);

/* ---- MMoE training ("Training") ---- */
/* rk_mlp_pack_weight of `count` weights in one launch per 96 of them (a train step repacks every
 * image it reads on the stream, so that a hipGraph replay follows the optimizer): out = the
 * [pad64(n), pad64(k)] image of w [n, k] (row stride ldw), 16-B aligned.                        */
typedef struct rk_pack_item {
  const float* w;
  float* out;
  int64_t ldw;
  int32_t n;
  int32_t k;
} rk_pack_item;
int rk_mlp_pack_weights(const rk_pack_item* items, int32_t count, void* stream);

/* rk_mmoe_forward in train mode, still one launch: dropout (probability dropout_p in [0, 1), scale
 * 1 / (1 - p)) behind every ReLU, and everything the backward reads kept.  Every hidden layer must be
 * ReLU, all experts (towers) must have the same widths layer by layer.  Dropout site s = e *
 * expert_depth + l for expert e layer l, num_experts * expert_depth + k * tower_depth + l for tower k
 * layer l; element (b, j) of a site's [batch, n] output is kept iff the counter hash of
 * rk_dropout_mask(seed + s, stream_slot, ...) keeps element b * n + j (stream_slot may be NULL
 * when dropout_p == 0).  With p4(v) = v rounded up to
 * a multiple of 4, the saved buffers (16-B aligned, columns between a width and its p4 zero) are
 *   x_out          [batch, p4(width)]                      the gathered rows
 *   expert_acts[l] [batch, num_experts * p4(n_l)]          expert e's layer l (after ReLU and dropout) at
 *                                                          columns e * p4(n_l); l = expert_depth - 1 is f_e
 *   tower_acts[l]  [batch, num_tasks * p4(n_l)]            tower k's layer l likewise
 *   mixed          [batch, num_tasks * p4(H)]              m_k at columns k * p4(H) (not [batch, K, H])
 *   gate_probs     [batch, num_tasks, num_experts]
 * mixed and gate_probs are required; logits / probs as in rk_mmoe_forward.  With dropout_p == 0 the
 * logits and probs have rk_mmoe_forward's bits.  Errors and envelope as rk_mmoe_forward.        */
int rk_mmoe_forward_train(const rk_segment* segs, int32_t nseg, int32_t width, int64_t batch,
                          const rk_mmoe_layer* experts, int32_t num_experts, int32_t expert_depth,
                          const float* gate_w, const float* gate_b, int32_t num_tasks,
                          const rk_mmoe_layer* towers, int32_t tower_depth, const float* const* head_w,
                          const float* const* head_b, double dropout_p, uint64_t seed,
                          const int64_t* stream_slot, float* x_out, float* const* expert_acts,
                          float* const* tower_acts, float* logits, float* probs, float* mixed,
                          float* gate_probs, void* stream);

/* Backward of the mix and of the gates' softmax, one launch, rows independent.  Per row b, with
 * dm_k = dmixed[b * ld_dmixed + k * pitch_dmixed ..] [H], f_e = f[b * ld_f + e * pitch_f ..] [H] (the
 * experts' last outputs after ReLU and dropout) and g = gate_probs[b] [num_tasks, num_experts]:
 *   dg[k][e] = sum_h dm_k[h] f_e[h]
 *   dgate_logits[b * ld_dgl + k * num_experts + e] = g[k][e] (dg[k][e] - sum_e' g[k][e'] dg[k][e'])
 *   dz[b * ld_dz + e * pitch_dz + h] = (sum_k g[k][e] dm_k[h]) * mask_scale * [f_e[h] > 0]   (h < H; zeros
 *                                                                                           up to pitch_dz)
 * Sums in a fixed order, no atomics.  With one expert the gate gradient is exactly 0.  Envelope:
 * num_experts <= 16, num_tasks <= 8, num_tasks * num_experts <= 64, H <= 512 (RK_ERR_UNSUPPORTED); NULL, a pitch or
 * leading dimension too small, a pointer not aligned to 4 B: RK_ERR_INVALID; both before any launch.
 * batch == 0: RK_OK, no launch.                                                                  */
int rk_mmoe_mix_backward(int64_t batch, int32_t num_experts, int32_t num_tasks, int32_t H, const float* dmixed,
                         int64_t ld_dmixed, int32_t pitch_dmixed, const float* f, int64_t ld_f, int32_t pitch_f,
                         const float* gate_probs, float mask_scale, float* dgate_logits, int64_t ld_dgl,
                         float* dz, int64_t ld_dz, int32_t pitch_dz, void* stream);

/* Backward of the num_tasks heads (Linear(n, 1) + sigmoid) into their inputs, one launch:
 *   g[b][k] = dlogits[b][k] + dprobs[b][k] p (1 - p)        (either gradient may be NULL, not both;
 *                                                            dlogits, dprobs, probs [batch, num_tasks])
 *   g_out[b * ld_g + k] = g[b][k]  (zeros for num_tasks <= k < ld_g)
 *   dt[b * num_tasks * pitch + k * pitch + j] (+)= g[b][k] head_w[k][j] (j < n; 0 up to pitch),
 *       times mask_scale * [t[same index] > 0] when t != NULL (the towers' last outputs).
 * The heads' dw / db are rk_gemm_wgrad(g_out, the towers' outputs): no sum over rows here.
 * num_tasks, ld_g <= 8 (RK_ERR_UNSUPPORTED); NULL / misaligned pointers: RK_ERR_INVALID.        */
int rk_mmoe_head_backward(int64_t batch, int32_t num_tasks, int32_t n, int32_t pitch, const float* dlogits,
                          const float* dprobs, const float* probs, const float* const* head_w, const float* t,
                          float mask_scale, float* g_out, int32_t ld_g, float* dt, int32_t accumulate,
                          void* stream);

/* ---- ESMM: entire space multi-task model (Ma et al., SIGIR 2018) ---- */
/* The whole ESMM eval forward in one launch.  Per row b, with x = the `width` columns gathered from
 * segs (rk_mmoe_forward's column map; out-of-range ids read zero rows and raise RK_FLAG_INDEX_OOB),
 * gathered once for all towers:
 *   logit_k = towers[k](x) . head_w[k] + head_b[k][0]    towers[k * tower_depth + l], l = 0 .. tower_depth - 1,
 *                                                        every tower reads the same x; head_w[k] [last width]
 *   cond_k  = sigmoid(logit_k)                           the conditional probability (pCTR, pCVR, ...)
 *   prob_k  = cond_0 cond_1 ... cond_k                   k ascending, FP32: the entire-space probability
 * Outputs, each may be NULL but not all: logits, probs, cond [batch, num_tasks], contiguous.  No tower
 * activation reaches memory; two launches give the same bits.
 * Envelope: nseg <= 16 segments of at most 255 columns each, width <= 256, 2 <= num_tasks <= 8,
 * 1 <= tower_depth <= 3, every n <= 512, activations none / ReLU (else RK_ERR_UNSUPPORTED); NULL or
 * shape errors, no output and batch < 0: RK_ERR_INVALID; both before any launch.  batch == 0: RK_OK,
 * no launch.                                                                                      */
int rk_esmm_forward(const rk_segment* segs, int32_t nseg, int32_t width, int64_t batch,
                    const rk_mmoe_layer* towers, int32_t num_tasks, int32_t tower_depth,
                    const float* const* head_w, const float* const* head_b, float* logits, float* probs,
                    float* cond, void* stream);

/* rk_esmm_forward in train mode, still one launch: dropout (probability dropout_p in [0, 1), scale
 * 1 / (1 - p)) behind every ReLU, and what the backward reads kept.  Every hidden layer must be ReLU and
 * all towers must have the same widths layer by layer.  Dropout site s = k * tower_depth + l for tower k
 * layer l; element (b, j) of a site's [batch, n] output is kept iff the counter hash of
 * rk_dropout_mask(seed + s, stream_slot, ...) keeps element b * n + j (stream_slot may be NULL when
 * dropout_p == 0).  Saved buffers (16-B aligned, p4 as in rk_mmoe_forward_train):
 *   x_out          [batch, p4(width)]               the gathered rows, zeros past the width
 *   tower_acts[l]  [batch, num_tasks * p4(n_l)]     tower k's layer l (after ReLU and dropout) at columns
 *                                                   k * p4(n_l), zeros up to the pitch:
 *                                                   rk_mmoe_forward_train's tower_acts layout
 * With dropout_p == 0 the outputs have rk_esmm_forward's bits.  Errors and envelope as rk_esmm_forward. */
int rk_esmm_forward_train(const rk_segment* segs, int32_t nseg, int32_t width, int64_t batch,
                          const rk_mmoe_layer* towers, int32_t num_tasks, int32_t tower_depth,
                          const float* const* head_w, const float* const* head_b, double dropout_p, uint64_t seed,
                          const int64_t* stream_slot, float* x_out, float* const* tower_acts, float* logits,
                          float* probs, float* cond, void* stream);

/* The entire-space loss and its gradient.  logits [batch, num_tasks] (row stride ld_logits) are the
 * conditional logits z, labels [batch, num_tasks] (row stride ld_labels, floats in [0, 1]) the labels of
 * the joint events (click; click and conversion; ...), task_weights a HOST array w [num_tasks] or NULL
 * (ones).  With ls_j = logsigmoid(z_j) and S_k = ls_0 + ... + ls_k (= log prob_k):
 *   L_0 = softplus(-z_0) y_0 + softplus(z_0) (1 - y_0)
 *   L_k = -(y_k S_k + (1 - y_k) log1mexp(S_k)),  k >= 1;  log1mexp(s) = log(-expm1(s)) for s > -ln 2,
 *                                                          else log1p(-exp(s))
 *   loss[0]     = (1 / batch) sum_b sum_k w_k L_k                        (device scalar)
 *   per_task[k] = (1 / batch) sum_b L_k                                  (device [num_tasks], unweighted)
 *   dlogits[b * ld_dlogits + j] = d loss / d z_j
 *     = ([j == 0] (sigmoid(z_0) - y_0) w_0 + sigmoid(-z_j) sum_{k >= max(j, 1)} w_k ((1 - y_k) / expm1(-S_k) - y_k)) / batch
 * S_k is clamped to at most -FLT_MIN where it is the argument of expm1 or log1mexp, so every output is
 * finite for every finite logit.  Each of loss, per_task, dlogits may be NULL, not all.  Sums run in a
 * fixed order without atomics (a second, one-workgroup launch adds the workgroups' sums): two runs give
 * the same bits.  workspace: rk_esmm_loss_workspace_floats(batch) device floats.  batch == 0: loss and
 * per_task are written as 0.  num_tasks <= 8 (RK_ERR_UNSUPPORTED); NULL, a leading dimension below
 * num_tasks, a short workspace: RK_ERR_INVALID.                                                    */
int64_t rk_esmm_loss_workspace_floats(int64_t batch);
int rk_esmm_loss(const float* logits, int64_t ld_logits, const float* labels, int64_t ld_labels, int64_t batch,
                 int32_t num_tasks, const float* task_weights, float* loss, float* per_task, float* dlogits,
                 int64_t ld_dlogits, float* workspace, int64_t workspace_floats, void* stream);

/* Folds the gradients arriving at rk_esmm_forward's outputs onto the conditional logits, one launch:
 *   g[b * ld_g + j] = dlogits_j + s(z_j) s(-z_j) dcond_j + s(-z_j) sum_{k >= j} dprobs_k prob_k
 * with s = sigmoid and prob_k recomputed from logits [batch, num_tasks] (row stride ld_logits); no
 * division by a probability.  dlogits, dprobs, dcond [batch, num_tasks] (row stride ld_in) may each be
 * NULL, not all.  g then enters rk_mmoe_head_backward as its dlogits (dprobs = NULL).  num_tasks <= 8
 * (RK_ERR_UNSUPPORTED); NULL / size errors: RK_ERR_INVALID.  batch == 0: RK_OK, no launch.       */
int rk_esmm_joint_backward(const float* logits, int64_t ld_logits, const float* dlogits, const float* dprobs,
                           const float* dcond, int64_t ld_in, int64_t batch, int32_t num_tasks, float* g,
                           int64_t ld_g, void* stream);

/* ---- PLE: progressive layered extraction (Tang et al., RecSys 2020), eval forward ---- */
/* The whole PLE eval forward in one launch.  L = num_levels, K = num_tasks, ms = num_specific, mc =
 * num_shared, NE = K ms + mc stacks per level (task k's at k ms + i, the shared at K ms + i), De =
 * expert_depth, Dt = tower_depth, H = expert_units[De - 1].  Per row b, with x = the `width` columns
 * gathered from segs (as rk_mmoe_forward) and x_k^{-1} = x_s^{-1} = x, level j = 0 .. L - 1 computes
 *   f_s   = expert_{j,s}(its owner's input)       Linear + ReLU per expert_units entry; stack k ms + i reads
 *                                                 x_k^{j-1}, stack K ms + i reads x_s^{j-1}
 *   g_k   = softmax(gate_{j,k}(x_k^{j-1}))        ms + mc columns: c < ms -> f_{k ms + c}, else f_{K ms + c - ms}
 *   g_s   = softmax(gate_{j,K}(x_s^{j-1}))        NE columns: c -> f_c (not at the last level)
 *   x_k^j = sum_c g_k[c] f,  x_s^j = sum_c g_s[c] f      c ascending, FP32, no atomics: two launches give
 *                                                 the same bits
 * then logit_k = towers[k](x_k^{L-1}) . head_w[k] + head_b[k][0] (Linear + ReLU per tower_units entry),
 * prob_k = sigmoid(logit_k).
 * table: a DEVICE array of table_len rk_mmoe_layer from which only w and bias are read (every width
 * comes from expert_units / tower_units), w = the rk_mlp_pack_weight image, bias [n] or NULL:
 *   [(j NE + s) De + l]              expert s of level j, layer l
 *   [L NE De + j (K + 1) + q]        level j's gate q (q == K: the shared gate; unused at the last level)
 *   [L NE De + L (K + 1) + k Dt + l] tower k, layer l
 *   [.. + K Dt + k]                  head k: w = the plain weight [last width], bias [1], both required
 * so table_len = L NE De + L (K + 1) + K Dt + K (without heads: L NE De + L (K + 1)).  The table and everything it points to is the caller's
 * to keep valid and 16-B aligned; the host checks its length and address only.
 * Outputs, each may be NULL: logits, probs [batch, K] (need has_heads != 0); level_reps[j]
 * [batch, K + 1, H] (x_0 .. x_{K-1}, x_s; [batch, K, H] at the last level); level_gates[j]
 * [batch, K (ms + mc) + NE] (g_0 .. g_{K-1}, g_s; [batch, K (ms + mc)] at the last level); level_reps /
 * level_gates are host arrays of L pointers or NULL.  has_heads == 0 (then tower_depth = 0) stops after
 * the last level.
 * Envelope: nseg <= 16 segments of at most 255 columns each, width <= 256, L <= 4, K <= 8, ms >= 0,
 * mc >= 1, NE <= 64, 1 <= De <= 3, 0 <= Dt <= 3, every n <= 512, and the level inputs, activation
 * buffers, gates and K + 1 mixtures within 160 KiB of LDS (else RK_ERR_UNSUPPORTED); NULL or shape
 * errors and batch < 0: RK_ERR_INVALID; both before any launch.  batch == 0: RK_OK, no launch.
 * Out-of-range ids read zero rows and raise RK_FLAG_INDEX_OOB.                                     */
int rk_ple_forward(const rk_segment* segs, int32_t nseg, int32_t width, int64_t batch, int32_t num_levels,
                   int32_t num_tasks, int32_t num_specific, int32_t num_shared, const int32_t* expert_units,
                   int32_t expert_depth, const int32_t* tower_units, int32_t tower_depth, int32_t has_heads,
                   const rk_mmoe_layer* table, int64_t table_len, float* logits, float* probs,
                   float* const* level_reps, float* const* level_gates, void* stream);

/* ---- PLE training ("Training") ---- */
/* rk_ple_forward in train mode, still one launch: dropout (probability dropout_p in [0, 1), scale
 * 1 / (1 - p)) behind every ReLU, and everything the backward reads kept.  Dropout sites:
 *   expert s of level j, layer l    (j NE + s) De + l          (its index in the layer table)
 *   tower k, layer l                L NE De + k Dt + l
 * element (b, c) of a site's [batch, n] output is kept iff the counter hash of rk_dropout_mask(seed +
 * site, stream_slot, ...) keeps element b * n + c (stream_slot may be NULL when dropout_p == 0).  With
 * p4(v) = v rounded up to a multiple of 4, the saved buffers (all required, 16-B aligned, the columns
 * between a width and its p4 written as zeros) are
 *   x_out                   [batch, p4(width)]            the gathered rows
 *   expert_acts[j De + l]   [batch, NE * p4(n_l)]         level j: stack s's layer l (after ReLU and dropout)
 *                                                         at columns s * p4(n_l); l = De - 1 is f_s
 *   tower_acts[l]           [batch, K * p4(n_l)]          tower k's layer l at columns k * p4(n_l)
 *   level_reps[j]           [batch, (K + 1) * p4(H)]      mixture i at columns i * p4(H) ([batch, K * p4(H)] at
 *                                                         the last level; not rk_ple_forward's layout)
 *   level_gates[j]          rk_ple_forward's layout
 *   logits, probs           [batch, K], required with has_heads != 0
 * With dropout_p == 0 the logits, probs and every level's representations and gates have
 * rk_ple_forward's bits.  Envelope and errors as rk_ple_forward; in addition dropout_p outside [0, 1),
 * a NULL or misaligned saved buffer, or a NULL stream_slot with dropout_p > 0: RK_ERR_INVALID before
 * any launch.  batch == 0: RK_OK, no launch.                                                       */
int rk_ple_forward_train(const rk_segment* segs, int32_t nseg, int32_t width, int64_t batch, int32_t num_levels,
                         int32_t num_tasks, int32_t num_specific, int32_t num_shared, const int32_t* expert_units,
                         int32_t expert_depth, const int32_t* tower_units, int32_t tower_depth, int32_t has_heads,
                         const rk_mmoe_layer* table, int64_t table_len, double dropout_p, uint64_t seed,
                         const int64_t* stream_slot, float* x_out, float* const* expert_acts,
                         float* const* tower_acts, float* logits, float* probs, float* const* level_reps,
                         float* const* level_gates, void* stream);

/* Backward of one level's mixtures and gates, one launch, rows independent.  K = num_tasks, ms =
 * num_specific, mc = num_shared, NE = K ms + mc, nq = K + 1 mixtures (K when has_shared_mix == 0: the
 * last level).  s(i, c), the stack behind column c of gate i: i ms + c (c < ms) or K ms + c - ms for i < K,
 * c for i == K.  Per row b, with dm_i = dm[b * ld_dm + i * pitch_dm ..] [H], f_s = f[b * ld_f + s *
 * pitch_f ..] [H] (the stacks' last outputs after ReLU and dropout) and g_i the gate weights at
 * gates[b * ld_gates ..] in rk_ple_forward's level_gates layout:
 *   dg_i[c]  = sum_h dm_i[h] f_{s(i,c)}[h]
 *   dgate_logits[b * ld_dgl + gate_offsets[i] + c] = g_i[c] (dg_i[c] - sum_c' g_i[c'] dg_i[c'])
 *   dz[b * ld_dz + stack_offsets[s] + h] = (sum over the (i, c) with s(i, c) = s, i ascending, of g_i[c]
 *                                          dm_i[h]) * mask_scale * [f_s[h] > 0]
 * with zeros behind a gate's columns up to the next multiple of 4 and behind H up to pitch_dz.
 * gate_offsets [nq] and stack_offsets [NE] are host arrays (copied into the kernel arguments).  Sums in a
 * fixed order, no atomics: two launches give the same bits; a one-column gate's gradient is exactly 0.
 * Envelope: K <= 8, NE <= 64, H <= 512 (RK_ERR_UNSUPPORTED); NULL, a pitch, leading dimension or
 * offset that does not fit, a pointer not aligned to 4 B, batch < 0: RK_ERR_INVALID; both before any
 * launch, nothing is written.  batch == 0: RK_OK, no launch.                                       */
int rk_ple_mix_backward(int64_t batch, int32_t num_tasks, int32_t num_specific, int32_t num_shared,
                        int32_t has_shared_mix, int32_t H, const float* dm, int64_t ld_dm, int32_t pitch_dm,
                        const float* f, int64_t ld_f, int32_t pitch_f, const float* gates, int64_t ld_gates,
                        float mask_scale, float* dgate_logits, int64_t ld_dgl, const int32_t* gate_offsets,
                        float* dz, int64_t ld_dz, const int32_t* stack_offsets, int32_t pitch_dz, void* stream);

/* ---- xDeepFM training: the CIN's train forward, data backward and weight gradient ---- */
/* rk_cin_forward that also writes every layer's feature maps for the backward:
 *   maps[(b * hsum + off_k + n) * dim + d] = x^k[b, n, d],  hsum = sum layer_sizes   (16-B aligned,
 * batch * hsum * dim floats).  Every other argument, output and bit as rk_cin_forward.          */
int rk_cin_forward_train(const rk_segment* second_order, const rk_segment* first_order, int32_t num_fields,
                         int32_t dim, int64_t batch, const float* const* weights, const float* const* biases,
                         const int32_t* layer_sizes, int32_t num_layers, int32_t activation,
                         const float* out_w, const float* out_b, float* deep_in, int64_t ld_deep, float* fm1,
                         float* pooled, int64_t ld_pooled, float* cin_logit, float* maps, void* stream);

/* W [n, hprev * num_fields] (row stride ldw) transposed and field-major for rk_cin_backward: the
 * matrix A[i * pad16(hprev) + h][n] = W[n][h * num_fields + i], zero padded, in rk_cin_pack_weight's
 * tile order; out: num_fields * pad16(hprev) * pad16(n) floats, 16-B aligned.                    */
int rk_cin_pack_weight_t(const float* w, int64_t ldw, int32_t n, int32_t hprev, int32_t num_fields, float* out,
                         void* stream);

/* The CIN's data backward in one launch.  x0 [batch, ld_x0]: the rows (field i at column i * dim),
 * maps: rk_cin_forward_train's, weights_t[k]: rk_cin_pack_weight_t images.  The gradient of
 * pooled[b, j] is dpooled[b, j] (may be NULL) + dlogit[b] * out_w[j] (dlogit may be NULL; one of the
 * two is required).  Writes dx0 [batch, ld_dx0] (+ dx0_add [batch, ld_add] when given) and
 * dy[(b * hsum + off_k + n) * dim + d] = dL/dy^k (the pre-activation gradients rk_cin_wgrad reads;
 * ReLU's derivative is maps > 0).  FP32 MFMA, fixed summation order, no atomics.  Envelope, errors
 * and batch == 0 as rk_cin_forward; rows 16-B aligned with strides % 4 == 0.                     */
int rk_cin_backward(const float* x0, int64_t ld_x0, int32_t num_fields, int32_t dim, int64_t batch,
                    const float* const* weights_t, const int32_t* layer_sizes, int32_t num_layers,
                    int32_t activation, const float* maps, const float* dpooled, int64_t ld_dpooled,
                    const float* dlogit, const float* out_w, const float* dx0_add, int64_t ld_add, float* dx0,
                    int64_t ld_dx0, float* dy, void* stream);

/* dW_k [layer_sizes[k], layer_sizes[k-1] * num_fields] (contiguous) and dbias_k [layer_sizes[k]]
 * (dbias or dbias[k] may be NULL) of every layer from x0, maps and rk_cin_backward's dy: slabs of the
 * batch * dim reduction go to `workspace` (rk_cin_wgrad_workspace_floats: a fixed number of slabs,
 * independent of the batch) and are added in slab order.  batch == 0: zeroed gradients, RK_OK.   */
int64_t rk_cin_wgrad_workspace_floats(int32_t num_fields, const int32_t* layer_sizes, int32_t num_layers);
int rk_cin_wgrad(const float* x0, int64_t ld_x0, int32_t num_fields, int32_t dim, int64_t batch,
                 const int32_t* layer_sizes, int32_t num_layers, const float* maps, const float* dy,
                 float* const* dw, float* const* dbias, float* workspace, int64_t workspace_floats, void* stream);

/* ---- table-sharded DeepFM, the local steps around the all-to-alls (rankops.sharded; the
 * reference's DeepFM.forward, deepfm.py:121-151, runs on one device) ---- */
/* The index all-to-all's send buffer in one launch: slot q (fields in owner-major order) copies
 * idx[q][0..batch) as int32 to out[base[q] + b * stride[q]] (base = batch * start_r + j,
 * stride = F_r: blocks [r][b][f_r]).  An index outside [0, 2^31) is sent as -1, so the owner's
 * rk_shard_gather_rows writes a zero row and raises RK_FLAG_INDEX_OOB instead of wrapping. */
int rk_shard_pack_indices(const int64_t* const* idx, const int64_t* base, const int32_t* stride,
                          int32_t num_fields, int64_t batch, int32_t* out, void* stream);
/* The row all-to-all's send buffer for samples [b0, b0 + bc) of every source: out[s][b'][j][0..row_floats)
 * = packed row idx[(s * source_batch + b0 + b') * num_fields + j] of table j (tables[j]: packed
 * rk_fm_pack_table layout, src_ld >= row_floats, 16-B aligned; idx / out / dim fields unused).
 * Out-of-range indices write zero rows and raise RK_FLAG_INDEX_OOB. */
int rk_shard_gather_rows(const rk_segment* tables, int32_t num_fields, int32_t row_floats, const int32_t* idx,
                         int32_t num_sources, int64_t source_batch, int64_t b0, int64_t bc, float* out,
                         void* stream);

/* The split wire format of the row exchange (round 5): out per source s = [bc][j][dim] second-order
 * rows straight from second[j] (the [V, dim] nn.Embedding weight, src_ld >= dim, 16-B aligned), then
 * pad4(bc) floats: per sample the sum over j = 0..num_fields-1 (in order) of the first-order weight
 * first[j].src[row * first[j].src_ld].  dim % 4 == 0.  Out-of-range indices give zero
 * rows / weights and raise RK_FLAG_INDEX_OOB. */
int rk_shard_gather_rows_split(const rk_segment* second, const rk_segment* first, int32_t num_fields,
                               int32_t dim, const int32_t* idx, int32_t num_sources, int64_t source_batch,
                               int64_t b0, int64_t bc, float* out, void* stream);
/* rk_deepfm_forward with the first-order weight of field f read from first[f][r * first_ld[f]]
 * (r = the field's index, or the sample for a dense block) instead of the packed row's column dim;
 * first[f] == NULL contributes 0 (ShardedDeepFM's split rows: the owner's partial sum on its first
 * field).  Rows then need src_ld >= dim only. */
int rk_deepfm_forward_fo(const rk_segment* fields, const float* const* first, const int64_t* first_ld,
                         int32_t num_fields, int32_t dim, int64_t batch, const rk_mlp_layer* layers,
                         int32_t nlayers, const rk_epilogue* head, float* fm1, float* fm2, void* stream);

/* ---- table-sharded DeepFM, training (rankops.sharded).  The wire is the split
 * format above in both directions; fields are dealt round robin, field f on owner f % num_owners
 * at slot f / num_owners, so owner r holds F_r = F / P + (r < F % P) fields and its block of
 * [batch][F_r][dim] rows then pad4(batch) first-order floats follows the blocks of owners 0..r-1
 * (an owner without fields has no block).  dim % 4 == 0, at most 32 fields per owner, buffers
 * 16-B aligned; anything else returns RK_ERR_INVALID before any write.  batch == 0 returns RK_OK
 * without a launch. ---- */
/* Receiver, forward: recv (the P blocks as received from the row all-to-all) -> deep_in
 * [batch, num_fields * dim] in field order (ld_deep % 4 == 0), fm1[b] = the owners' first-order
 * partials added in owner order, fm2[b] = 0.5 * sum_d ((sum_f e)^2 - sum_f e^2). */
int rk_shard_fm_assemble(const float* recv, int32_t num_fields, int32_t num_owners, int32_t dim,
                         int64_t batch, float* deep_in, int64_t ld_deep, float* fm1, float* fm2,
                         void* stream);
/* Receiver, backward: rk_fm_backward's gradient, times scale, written straight into the gradient
 * send buffer `out` (the same P blocks): row (b, f) = scale * (d_deep[b, f dim + d] + dfm2[b] *
 * (S_d - e[b, f, d])), S_d summed in field order from deep_in; every owner's tail gets
 * scale * dfm1[b], its pad lanes zeros.  d_deep and dfm2 may be NULL (zero). */
int rk_shard_fm_backward_pack(const float* deep_in, int64_t ld_in, const float* d_deep, int64_t ld_d,
                              const float* dfm2, const float* dfm1, float scale, int64_t batch,
                              int32_t num_fields, int32_t num_owners, int32_t dim, float* out,
                              void* stream);
/* Owner, backward: recv = the gradient blocks of every source s for this owner's num_fields
 * tables ([source_batch][num_fields][dim] rows then pad4(source_batch) first-order gradients per
 * source), idx = the int32 indices kept from the forward [s][b][j].  With N = num_sources *
 * source_batch and i = s * source_batch + b:  ids[j * N + i] = idx[s][b][j] widened (-1 stays -1),
 * values2[(j * N + i) * dim ..] = the row, values1[i] = the tail value (shared by the first-order
 * gradients of all the tables).  num_fields == 0 returns RK_OK without a launch. */
int rk_shard_unpack_grads(const float* recv, const int32_t* idx, int32_t num_fields, int32_t dim,
                          int32_t num_sources, int64_t source_batch, int64_t* ids, float* values2,
                          float* values1, void* stream);

/* FwFM.forward (fwfm.py:114-139): per sample, logit = sum_f linear[f] row + sum_{i<j} field_weight[p]
 * <embeddings[i] row, embeddings[j] row> + bias[0] (p runs i-major over i < j, fwfm.py:129-136),
 * prob = sigmoid(logit).  embeddings[f]: table segments of width dim (out_col ignored);
 * linear[f]: the first-order tables (dim 1).  2 <= num_fields <= 16, 1 <= dim <= 256 (dim > 64
 * needs 16-byte aligned rows).  logit may be NULL.  Out-of-range indices read zero rows and raise
 * RK_FLAG_INDEX_OOB.                                                                             */
int rk_fwfm_forward(const rk_segment* embeddings, const rk_segment* linear, int32_t num_fields,
                    int32_t dim, int64_t batch, const float* field_weight, const float* bias,
                    float* logit, float* prob, void* stream);

/* ---- training (§8(f) #2) ---------------------------------------------------------------- */
/* C[m, n] (+)= sum_r opA(m, r) * opB(n, r) on FP32 MFMA, with
 *   opA(m, r) = trans_a ? A[r*lda + m] : A[m*lda + r], times [A_mask(m, r) > 0] when A_mask
 *               (same layout and lda as A: the ReLU backward dz = dh * [h > 0]) is non-NULL;
 *   opB(n, r) = trans_b ? B[r*ldb + n] : B[n*ldb + r];
 *   row_sums[m] (+)= sum_r opA(m, r) when non-NULL (bias gradients).
 * nn.Linear backward: dX = dZ W  -> rk_gemm(0, 1, B, K, N, dZ, ldz, mask, W, K, dX, ...);
 *                     dW = dZ^T X -> rk_gemm(1, 1, N, K, B, dZ, ldz, mask, X, ldx, dW, K, db, ...).
 * split <= 0 picks a reduction split (float atomics) that fills the GPU; accumulate = 0
 * overwrites C / row_sums.                                                                  */
int rk_gemm(int32_t trans_a, int32_t trans_b, int64_t M, int64_t N, int64_t R, const float* A,
            int64_t lda, const float* A_mask, const float* B, int64_t ldb, float* C, int64_t ldc,
            float* row_sums, int32_t accumulate, int32_t split, void* stream);

/* Weight-gradient GEMM (every nn.Linear's dW / db in loss.backward(), e.g. bst.py:59-64,73-90,
 * dcn.py:147-150): C[n, k] (+)= sum_r opA(r, n) B[r * ldb + k] and row_sums[n] (+)= sum_r opA(r, n),
 * opA(r, n) = A[r * lda + n] (times [A_mask[r * lda + n] > 0] when A_mask != NULL), for a long
 * reduction R.  Same result as rk_gemm(1, 1, N, K, R, ...) but each 128 x 128 output tile is owned
 * by one workgroup per row slab and the slabs' partials are summed in a fixed order
 * (deterministic).  Needs N, K, lda, ldb, ldc % 4 == 0 and 16-B aligned pointers
 * (RK_ERR_UNSUPPORTED otherwise); workspace: rk_gemm_wgrad_workspace_floats(N, K, R) floats.  */
int rk_gemm_wgrad(int64_t N, int64_t K, int64_t R, const float* A, int64_t lda, const float* A_mask,
                  const float* B, int64_t ldb, float* C, int64_t ldc, float* row_sums,
                  int32_t accumulate, float* workspace, int64_t workspace_floats, void* stream);
int64_t rk_gemm_wgrad_workspace_floats(int64_t N, int64_t K, int64_t R);

/* G <= 16 GEMMs of one shape in one launch (the data gradients of G independent Linears): for every
 * group g, C[g][m * ldc + n] (+)= sum_r opA_g(m, r) opB_g(n, r) with rk_gemm's operand layouts, then
 * the *output* mask when C_mask != NULL: the product is multiplied by mask_scale * [C_mask[g][m *
 * ldmask + n] > 0] before it is stored (or added), so a masked dz buffer is formed once.  A, B, C, C_mask are
 * host arrays of G device pointers (copied into the kernel arguments); groups may be column blocks
 * of one wider buffer (ldc > N).  The whole reduction runs in one workgroup: no split, no atomics.
 * trans_a must be 0 (a transposed A is a weight gradient: rk_gemm_wgrad_grouped).  G > 16 or trans_a != 0:
 * RK_ERR_UNSUPPORTED; a NULL array or entry, a pointer not aligned to 4 B, a leading
 * dimension too small: RK_ERR_INVALID; nothing is written in either case.                       */
int rk_gemm_grouped(int32_t G, int32_t trans_a, int32_t trans_b, int64_t M, int64_t N, int64_t R,
                    const float* const* A, int64_t lda, const float* const* B, int64_t ldb, float* const* C,
                    int64_t ldc, const float* const* C_mask, int64_t ldmask, float mask_scale,
                    int32_t accumulate, void* stream);

/* rk_gemm_wgrad over G <= 16 groups of one shape in two launches (partials, fixed-order reduce):
 * C[g][n * ldc + k] (+)= sum_r A[g][r * lda + n] B[g][r * ldb + k], row_sums[g][n] (+)= sum_r A[g][r *
 * lda + n] (row_sums NULL: none).  Deterministic, no atomics; alignment rules and error codes as
 * rk_gemm_wgrad, G > 16 RK_ERR_UNSUPPORTED; workspace: rk_gemm_wgrad_grouped_workspace_floats.  */
int rk_gemm_wgrad_grouped(int32_t G, int64_t N, int64_t K, int64_t R, const float* const* A, int64_t lda,
                          const float* const* B, int64_t ldb, float* const* C, int64_t ldc,
                          float* const* row_sums, int32_t accumulate, float* workspace,
                          int64_t workspace_floats, void* stream);
int64_t rk_gemm_wgrad_grouped_workspace_floats(int32_t G, int64_t N, int64_t K, int64_t R);

/* out[i] (+)= dy[i] * [y[i] > 0] over n contiguous floats (ReLU backward from its output; the
 * residual path of residual_unit, deepcrossing.py:41).                                        */
int rk_relu_backward(const float* dy, const float* y, float* out, int64_t n, int32_t accumulate,
                     void* stream);

/* Linear(ka + kb, 1) + sigmoid head over rows [xa | xb] (kb may be 0):
 * g = dlogit + dprob * (1 - prob) * prob (either grad may be NULL); dxa/dxb = g w (NULL: not
 * written); dw[ka + kb] = sum_b g x; db[0] = sum_b g (both overwritten); g_out[b] = g.       */
int rk_logit_head_backward(const float* dlogit, const float* dprob, const float* prob, int64_t batch,
                           const float* xa, int64_t ld_xa, int32_t ka, const float* xb, int64_t ld_xb,
                           int32_t kb, const float* w, float* dxa, int64_t ld_dxa, float* dxb,
                           int64_t ld_dxb, float* dw, float* db, float* g_out, void* stream);

/* nn.Embedding gradient of a behaviour sequence without sorting (bst.py:224): grad[idx[b*stride + t]]
 * += dx[b*T + t, out_col : out_col + dim] for b < batch, t < T (grad->idx_stride = the row stride
 * of the [batch, T] index matrix).  Runs of equal consecutive ids in a sample (a padded tail) are
 * summed before their atomics.  Needs an even dim <= 128 and 8-B aligned rows
 * (RK_ERR_UNSUPPORTED otherwise: use rk_embedding_backward_sorted).                            */
int rk_embedding_backward_seq(const rk_segment* grad, int64_t batch, int32_t T, const float* dx,
                              int64_t ld_dx, void* stream);
/* Sorted segment-reduce form of rk_embedding_backward for ONE table segment and a long index list
 * with hot rows (padded behaviour sequences): grad[idx[i]] += dx[i, out_col:+dim] for i < n, via a
 * radix sort of the indices and one atomic per (distinct row in a 64-position chunk, column).
 * workspace: rk_embedding_backward_sorted_workspace_size(n) bytes.  Out-of-range indices are skipped
 * and raise RK_FLAG_INDEX_OOB.                                                               */
int rk_embedding_backward_sorted_workspace_size(int64_t n, int64_t* bytes);
int rk_embedding_backward_sorted(const rk_segment* grad, int64_t n, const float* dx, int64_t ld_dx,
                                 void* workspace, int64_t ws_bytes, void* stream);

/* Gradient of num_layers cross layers (rk_dcn_cross's stack, weights [L, width]) w.r.t. x0 given
 * dL/dx_L; written to dx0 (added when accumulate).  width <= 256, num_layers <= 8.           */
int rk_dcn_cross_backward(const float* x0, int64_t ld_x0, int64_t batch, int32_t width,
                          const float* cross_w, const float* cross_b, int32_t num_layers,
                          const float* dxl, int64_t ld_dxl, float* dx0, int64_t ld_dx0,
                          int32_t accumulate, void* stream);

/* Dense nn.Embedding weight gradients: for every table segment (src = the [rows, dim] gradient
 * buffer, written with float atomics — zero it first), grad[idx[b]] += dx[b, out_col:+dim].
 * Dense segments (idx == NULL) are skipped; out-of-range indices raise RK_FLAG_INDEX_OOB.   */
int rk_embedding_backward(const rk_segment* grads, int32_t nseg, int64_t batch, const float* dx,
                          int64_t ld_dx, void* stream);

/* Dropout streams: *slot = *counter; *counter += 1 (one thread, stream-ordered, graph-safe). */
int rk_rng_next(int64_t* counter, int64_t* slot, void* stream);

/* The keep mask a dropout stream draws, as the multiplier it applies: out[b*n + j] = 1/(1-p) or 0.
 * keep(i) = mix64(seed, *stream_slot, i) >= p * 2^32 (splitmix64 finaliser; not torch's Philox). */
int rk_dropout_mask(uint64_t seed, const int64_t* stream_slot, int64_t batch, int32_t n,
                    double dropout_p, float* out, void* stream);

/* y = Dropout_p(act(BatchNorm1d_train(z + bias))) over [batch, n] (deepfm.py:101-108; BST's
 * LeakyReLU units bst.py:207-211): batch statistics (biased variance) in fp64, save_mean /
 * save_invstd written, running_mean / running_var updated with momentum and the unbiased variance
 * (both may be NULL); batch_norm = 0 skips the normalisation, act = RK_ACT_NONE / RK_ACT_RELU /
 * RK_ACT_LEAKY (negative slope `slope`), dropout_p = 0 the dropout.  workspace: 2n doubles.
 * gamma / beta may be NULL (affine = False).                                                  */
int rk_bn_act_train_forward(const float* z, int64_t ldz, int64_t batch, int32_t n, const float* bias,
                            int32_t batch_norm, const float* gamma, const float* beta, float eps,
                            float momentum, float* running_mean, float* running_var,
                            double* workspace, float* save_mean, float* save_invstd, int32_t act,
                            float slope, double dropout_p, uint64_t seed, const int64_t* stream_slot, float* y,
                            int64_t ldy, void* stream);

/* Backward of rk_bn_act_train_forward given dy: dz (gradient w.r.t. z, i.e. the Linear output
 * before its bias), dgamma / dbeta (may be NULL).  Same seed / stream slot as the forward.    */
int rk_bn_act_backward(const float* dy, int64_t lddy, const float* z, int64_t ldz, int64_t batch,
                       int32_t n, const float* bias, int32_t batch_norm, const float* gamma,
                       const float* beta, const float* save_mean, const float* save_invstd,
                       int32_t act, float slope, double dropout_p, uint64_t seed,
                       const int64_t* stream_slot,
                       double* workspace, float* dz, int64_t lddz, float* dgamma, float* dbeta,
                       void* stream);

/* DeepFM FM backward (deepfm.py:122-140): out[b, f*dim + d] = d_deep[b, f*dim + d] +
 * dfm2[b] * (S_d - e_{f,d}), e = the saved deep input (concatenated second-order rows),
 * S_d = sum_f e_{f,d}.  d_deep / dfm2 may be NULL (zero).                                      */
int rk_fm_backward(const float* deep_in, int64_t ld_in, const float* d_deep, int64_t ld_d,
                   const float* dfm2, int64_t batch, int32_t num_fields, int32_t dim, float* out,
                   int64_t ld_out, void* stream);

/* final_layer(cat[fm1, fm2, deep]) + sigmoid backward (deepfm.py:147-150) with incoming grads of
 * all five outputs (each may be NULL): g = dtotal + dprob (1 - p) p; dfm1 = dfm1_in + g w0,
 * dfm2 = dfm2_in + g w1, ddeep = ddeep_in + g w2; dfinal_w[3], dfinal_b[1] overwritten.        */
int rk_fm_combine_backward(const float* dprob, const float* dtotal, const float* dfm1_in,
                           const float* dfm2_in, const float* ddeep_in, const float* prob,
                           const float* fm1, const float* fm2, const float* deep,
                           const float* final_w, int64_t batch, float* dfm1, float* dfm2,
                           float* ddeep, float* dfinal_w, float* dfinal_b, void* stream);

/* Dice (din.py:26-36) in train mode: x = z + bias, xhat = BatchNorm1d(affine=False) with the batch
 * statistics (running stats updated with momentum), y = alpha * (1 - sigmoid(xhat)) * x +
 * sigmoid(xhat) * x.  workspace: 2n doubles (forward), 3n (backward).  Backward writes dz =
 * dL/d(z + bias) and dalpha (when non-NULL).                                                  */
int rk_dice_train_forward(const float* z, int64_t ldz, int64_t batch, int32_t n, const float* bias,
                          const float* alpha, float eps, float momentum, float* running_mean,
                          float* running_var, double* workspace, float* save_mean, float* save_invstd,
                          float* y, int64_t ldy, void* stream);
int rk_dice_backward(const float* dy, int64_t lddy, const float* z, int64_t ldz, int64_t batch,
                     int32_t n, const float* bias, const float* alpha, const float* save_mean,
                     const float* save_invstd, double* workspace, float* dz, int64_t lddz,
                     float* dalpha, void* stream);

/* DIN's PReLU activation option (din.py:277-279, nn.PReLU()) in train mode: x = z + bias,
 * y = x > 0 ? x : a x, with one shared weight (num_weights == 1, the reference's nn.PReLU()) or
 * one per column (num_weights == n).  Backward writes dz = dL/d(z + bias) and dweight[num_weights]
 * (when non-NULL); workspace: num_weights doubles.                                              */
int rk_prelu_train_forward(const float* z, int64_t ldz, int64_t batch, int32_t n, const float* bias,
                           const float* weight, int32_t num_weights, float* y, int64_t ldy, void* stream);
int rk_prelu_backward(const float* dy, int64_t lddy, const float* z, int64_t ldz, int64_t batch,
                      int32_t n, const float* bias, const float* weight, int32_t num_weights,
                      double* workspace, float* dz, int64_t lddz, float* dweight, void* stream);

/* din_attention train pieces (din.py:42-84).  keys [B, T, H] = key_table[seq] (gathered), cross
 * [B*T, 4H] = [q, k, q-k, q*k] with q = x[b, q_col:+H]; the att_net layers run on rk_linear.
 * pool_forward: s = a2 . w3 + b3, masked (softmax: padded with -2^32+1, / sqrt(H)) weights saved
 * to weights [B, T], out = sum_t w_t k_t written to x[b, att_col:+H].  T <= 1024, H <= 64.
 * pool_backward: from dout = dx[b, att_col:+H]: dkeys = w_t dout (overwritten) and
 * da2 = ds_t w3 [a2 > 0].  cross_fold: d(cross) -> dq added to dx[b, q_col:+H], dkeys added.  */
int rk_din_att_cross(const float* x, int64_t ldx, int32_t q_col, const float* key_table,
                     int64_t key_rows, int64_t ld_key, const int64_t* seq, int64_t ld_seq,
                     int64_t batch, int32_t T, int32_t H, float* keys, float* cross, void* stream);
int rk_din_att_pool_forward(const float* a2, int32_t a2_width, const float* w3, const float* b3,
                            const float* keys, const int64_t* seq_len, int64_t batch, int32_t T,
                            int32_t H, int32_t use_softmax, float* weights, float* x, int64_t ldx,
                            int32_t att_col, void* stream);
int rk_din_att_pool_backward(const float* dx, int64_t lddx, int32_t att_col, const float* weights,
                             const float* keys, const float* a2, int32_t a2_width, const float* w3,
                             const int64_t* seq_len, int64_t batch, int32_t T, int32_t H,
                             int32_t use_softmax, float* dkeys, float* da2, void* stream);
int rk_din_cross_fold(const float* dcross, const float* x, int64_t ldx, int32_t q_col,
                      const float* keys, int64_t batch, int32_t T, int32_t H, float* dkeys, float* dx,
                      int64_t lddx, void* stream);

/* Backward of out = scale * mean_r ||x[r, col0:+ncols]||_2 (rk_row_l2norm_mean): called with
 * scale / rows, adds grad_out[0] * scale * x / ||x_r|| to dx[r, col0 + c] (0 for a zero row).   */
int rk_row_l2norm_backward(const float* x, int64_t ldx, int64_t rows, int32_t col0, int32_t ncols,
                           float scale, const float* grad_out, float* dx, int64_t lddx, void* stream);

/* FwFM backward from dL/dprob [B] (BCELoss on rk_fwfm_forward's probabilities, fwfm.py:150-156):
 * dz = dprob * (1 - prob) * prob -> dz [B] (the first-order tables' gradient rows),
 * d_emb[b, f*dim + c] = dz * sum_{j != f} r_{pair(f,j)} E_j[c] (scatter with rk_embedding_backward),
 * d_field_weight [F(F-1)/2] and d_bias [1] (overwritten).                                   */
int rk_fwfm_backward(const rk_segment* embeddings, int32_t num_fields, int32_t dim, int64_t batch,
                     const float* field_weight, const float* prob, const float* dprob, float* d_emb,
                     int64_t ld_demb, float* dz, float* d_field_weight, float* d_bias, void* stream);

/* AFM training (afm.py:92-119).  pairs: emb [B, F*dim] (gathered rows) and pairs [B*P, dim]
 * (P = F(F-1)/2, i-major), 2 <= F <= 16.  The attention's first layer a1 = relu(pairs W1^T + b1)
 * runs on rk_linear; pool_forward: s = a1 . w2 + b2, softmax over the P pairs (weights [B, P]),
 * ws = sum_p w_p pair_p [B, dim], logit = dense . wd + bd + ws . wp + bp, pred = sigmoid(logit)
 * (dim, num_dense <= 64; logit may be NULL).  pool_backward from dpred and/or dtotal (either may
 * be NULL): d_pairs (direct part, overwritten), da1 = d a1 [B*P, A] (masked by a1 > 0), and
 * acc = [d wd (num_dense) | d bd | d wp (dim) | d bp | d w2 (A <= 256) | d b2] (overwritten).
 * pair_fold: d_emb[b, i*dim + d] = sum_j d_pairs[b, pair(i,j), d] * emb[b, j*dim + d].          */
int rk_afm_pairs(const rk_segment* fields, int32_t num_fields, int32_t dim, int64_t batch, float* emb,
                 float* pairs, void* stream);
int rk_afm_pool_forward(const float* a1, int32_t att_dim, const float* w2, const float* b2,
                        const float* pairs, int32_t num_pairs, int32_t dim, const float* dense,
                        int64_t ld_dense, int32_t num_dense, const float* wd, const float* bd,
                        const float* wp, const float* bp, int64_t batch, float* weights, float* ws,
                        float* logit, float* pred, void* stream);
int rk_afm_pool_backward(const float* dpred, const float* dtotal, const float* pred,
                         const float* weights, const float* ws, const float* pairs, const float* a1,
                         int32_t att_dim, const float* w2, const float* wp, const float* dense,
                         int64_t ld_dense, int32_t num_dense, int64_t batch, int32_t num_pairs,
                         int32_t dim, float* d_pairs, float* da1, float* acc, void* stream);
int rk_afm_pair_fold(const float* d_pairs, const float* emb, int32_t num_fields, int32_t dim,
                     int64_t batch, float* d_emb, void* stream);

/* BST training (bst.py:66-91, 238-241), rows = B*T of width d:
 *   add_pos: xp[m] = x[m] + pos[m % T].
 *   attn_train_forward: per (sample, head) P = softmax(mask(Q K^T / sqrt(dh))) saved to probs (or not
 *     saved when probs == NULL; T % 4 == 0, dh % 4 == 0)
 *     [B, heads, T, T] and ctx = P V [rows, d]; qkv is [rows, 3d] = [Q | K | V].  T <= 64,
 *     d / heads <= 64.  attn_train_backward: dqkv [rows, 3d] from dctx (overwritten).
 *   res_dropout_ln_forward: r = base + Dropout_p(o) (saved), y = LayerNorm(r) (gamma, beta, eps),
 *     mean / rstd [rows] saved.  d <= 256.
 *   ln_backward: dr = LayerNorm backward of dy (overwritten), d_o = Dropout_p-masked dr (NULL:
 *     skipped), dgamma / dbeta [d] (overwritten, summed in a fixed order: workspace 1024 * d floats).
 *   pos_backward: dpos[t] += sum_b dxp[b*T + t] for t < T (the position-embedding gradient; zero dpos first).
 *   leaky_dropout: forward out = Dropout_p(LeakyReLU_slope(f)); backward (backward = 1)
 *     out = in * keep * scale * (f > 0 ? 1 : slope).
 *   pool: row[b, col:+d] = sum_t x[b*T + t] (/ seq_len[b] when mean); pool_backward broadcasts.
 * Dropout masks: the counter hash of rk_dropout_mask with index m * d + k.                      */
int rk_bst_add_pos(const float* x, const float* pos, int32_t T, int64_t rows, int32_t d, float* xp,
                   void* stream);
/* Behaviour-sequence gather + position add of the first block's train forward (bst.py:224,73-75):
 * x[m] = table[idx[m]] (out-of-range: zeros + RK_FLAG_INDEX_OOB), xp[m] = x[m] + pos[m % T, :].
 * Needs d % 4 == 0 and 16-B aligned rows (RK_ERR_UNSUPPORTED otherwise).                       */
int rk_bst_gather_pos(const float* table, int64_t rows, int64_t ld_table, const int64_t* idx,
                      int64_t n, int32_t T, int32_t d, const float* pos, float* x, float* xp,
                      void* stream);
int rk_bst_attn_train_forward(const float* qkv, int64_t batch, int32_t T, int32_t d, int32_t heads,
                              const int64_t* seq_len, float* probs, float* ctx, void* stream);
int rk_bst_attn_train_backward(const float* qkv, const float* probs, const float* dctx,
                               int64_t batch, int32_t T, int32_t d, int32_t heads, float* dqkv,
                               void* stream);
/* The O / FFN2 projection and the residual LayerNorm after it in one launch (bst.py:84-90):
 * r = base + dropout(x W^T + bias), y = LayerNorm(r) (gamma, beta, eps), mean / rstd per row, for
 * d_model = N = 128: the projection output never reaches HBM.  x [M, K] (ld ldx), W [128, K] (ld
 * ldw), base / r / y [M, 128] contiguous; K in {32, 64, 128}, 16-B aligned rows
 * (RK_ERR_UNSUPPORTED otherwise: use rk_linear + rk_bst_res_dropout_ln_forward).
 * Same dropout mask as rk_bst_res_dropout_ln_forward for the same (seed, stream slot).          */
int rk_linear_res_dropout_ln(const float* x, int64_t ldx, int64_t M, int32_t K, const float* w, int64_t ldw,
                             const float* bias, const float* base, double dropout_p, uint64_t seed,
                             const int64_t* stream_slot, const float* gamma, const float* beta, float eps,
                             float* r, float* y, float* mean, float* rstd, void* stream);
int rk_bst_res_dropout_ln_forward(const float* base, const float* o, int64_t rows, int32_t d,
                                  double dropout_p, uint64_t seed, const int64_t* stream_slot,
                                  const float* gamma, const float* beta, float eps, float* r, float* y,
                                  float* mean, float* rstd, void* stream);
int rk_bst_ln_backward(const float* dy, const float* r, const float* mean, const float* rstd,
                       const float* gamma, int64_t rows, int32_t d, double dropout_p, uint64_t seed,
                       const int64_t* stream_slot, float* dr, float* d_o, float* dgamma, float* dbeta,
                       float* workspace, int64_t workspace_floats, void* stream);
/* rk_bst_ln_backward of the last block fused with the pooling backward (bst.py:238-241): the
 * incoming gradient of row m is drow[m / T, col:col+d] (/ seq_len[m / T] when mean_pool), so the
 * [rows, d] broadcast is never written.  rows = batch * T; needs d % 4 == 0 and 16-B aligned r /
 * dr / d_o rows (drow any alignment; RK_ERR_UNSUPPORTED otherwise: use rk_bst_pool_backward +
 * rk_bst_ln_backward).                                                                         */
int rk_bst_pool_ln_backward(const float* drow, int64_t ld_row, int32_t col, int32_t T,
                            const int64_t* seq_len, int32_t mean_pool, const float* r,
                            const float* mean, const float* rstd, const float* gamma, int64_t rows,
                            int32_t d, double dropout_p, uint64_t seed, const int64_t* stream_slot,
                            float* dr, float* d_o, float* dgamma, float* dbeta, float* workspace,
                            int64_t workspace_floats, void* stream);
/* Floats rk_bst_ln_backward / rk_bst_pool_ln_backward need in `workspace` for model width d. */
int64_t rk_bst_ln_backward_workspace_floats(int32_t d);
int rk_bst_pos_backward(const float* dxp, int64_t batch, int32_t T, int32_t d, float* dpos, void* stream);
int rk_bst_leaky_dropout(const float* in, const float* f, int64_t n, float slope, double dropout_p,
                         uint64_t seed, const int64_t* stream_slot, int32_t backward, float* out,
                         void* stream);
int rk_bst_pool(const float* x, int64_t batch, int32_t T, int32_t d, const int64_t* seq_len,
                int32_t mean, float* row, int64_t ld_row, int32_t col, void* stream);
int rk_bst_pool_backward(const float* drow, int64_t ld_row, int32_t col, int64_t batch, int32_t T,
                         int32_t d, const int64_t* seq_len, int32_t mean, float* dx, void* stream);

typedef struct rk_adam_tensor {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t numel;
  float* step; /* optional device step counter (torch capturable=True): incremented on the device,
                  bias corrections formed there; give it for all tensors of a call or for none */
} rk_adam_tensor;

/* One torch.optim.Adam step (amsgrad = maximize = False; L2 weight_decay added to the gradient)
 * for every tensor in the list; `step` is the 1-based step count after increment (ignored when
 * the tensors carry device step counters: then the call is graph-capturable).  Scalars are
 * doubles (Python floats): derived values (1 - beta, lr / bias_correction1, ...) are formed in
 * double and rounded to float once, as torch does.                                            */
int rk_adam_step(const rk_adam_tensor* tensors, int32_t n, double lr, double beta1, double beta2,
                 double eps, double weight_decay, int64_t step, void* stream);

typedef struct rk_sparse_adam_tensor {
  float* param;       /* [rows, dim] table, row stride ld (floats) */
  float* exp_avg;     /* same shape and stride */
  float* exp_avg_sq;
  int64_t rows;
  int64_t ld;
  const int64_t* idx; /* nnz row ids of the sparse gradient, element i at idx[i * idx_stride]; any
                         order, duplicates allowed */
  int64_t idx_stride;
  int64_t nnz;
  const float* values; /* [nnz, dim] gradient rows, row stride ld_values (floats) */
  int64_t ld_values;
  int32_t dim;         /* any dim >= 1 */
  int32_t coalesced;   /* non-zero: idx is ascending without duplicates (a coalesced COO tensor);
                          such tables skip the sort.  A list flagged wrongly gives wrong sums for
                          its duplicated rows, never a fault */
} rk_sparse_adam_tensor;

/* One torch.optim.SparseAdam step (= TF LazyAdamOptimizer's arithmetic, DIEN/dien.py:328) for
 * every table in the list: for each distinct row r of a table's gradient, g = the sum of the
 * row's entries (in list order: no float atomics, equal inputs give equal bits), then
 *   m += (1 - beta1) (g - m);  v += (1 - beta2) (g^2 - v);
 *   p -= lr sqrt(1 - beta2^t) / (1 - beta1^t) * m / (sqrt(v) + eps)
 * Rows that are not in the gradient are neither read nor written.  `step` is the 1-based count t
 * after increment; when device_step is given (a float counter in device memory, torch's
 * capturable layout) it is incremented on the device instead, t is read from it and `step` is
 * ignored: the call is then graph-capturable.  Scalars are doubles, derived values are formed in
 * double and rounded to float once, as in rk_adam_step.
 * An id outside [0, rows) never faults: its entry contributes nothing and RK_FLAG_INDEX_OOB is
 * raised (rk_error_flags).  A table of 2^32 rows or more, or of more than 2^32 - 513 entries, is
 * RK_ERR_UNSUPPORTED.  Launches per call do not depend on the number of tables while they fit one
 * group: up to 64 tables whose rows together fit 32-bit keys (the radix sort runs over the bits
 * the group needs); more tables or rows make further groups.  Tables with nnz 0 are skipped.
 * workspace: rk_sparse_adam_step_workspace_size bytes of device memory for the same list, owned
 * by the caller and free for reuse once the call's work on `stream` has run.                    */
int rk_sparse_adam_step_workspace_size(const rk_sparse_adam_tensor* tensors, int32_t n, int64_t* bytes);
int rk_sparse_adam_step(const rk_sparse_adam_tensor* tensors, int32_t n, double lr, double beta1, double beta2,
                        double eps, int64_t step, float* device_step, void* workspace, int64_t ws_bytes,
                        void* stream);

/* Packs column blocks of row-major matrices into contiguous buffers, all blocks in one launch
 * (the value rows of sparse embedding gradients out of a backward's dx): for block k,
 * dst[k][b * dim[k] + c] = src[k][b * ld_src[k] + c] (+ add[k][b * ld_add[k] + c] when add is
 * given: a gradient kept as two summands) for b < rows[k], c < dim[k].                          */
typedef struct rk_pack_block {
  const float* src;
  const float* add; /* optional second summand, NULL for a plain copy */
  float* dst;
  int64_t ld_src;
  int64_t ld_add;
  int64_t rows;
  int32_t dim;
  int32_t reserved;
} rk_pack_block;
int rk_pack_blocks(const rk_pack_block* blocks, int32_t n, void* stream);

/* ---- evaluation metrics (the reference's evaluate(): dcn.py:214-239, same in every model) ---- */
/* One batch into accum (3 x 8 bytes, zero it first): [0] double sum over batches of the batch's
 * mean loss — loss_kind 0: BCEWithLogitsLoss(logits, labels) (dcn.py:229, bst.py:300,
 * deepcrossing.py:212); 1: BCELoss(probs, labels), logs clamped at -100 (din.py:379, deepfm.py:198,
 * afm.py:203, fwfm.py:176; logits may be NULL) — plus *extra if non-NULL (DIN's l2_reg, din.py:380);
 * [1] uint64 count of rint(probs) == labels (accuracy_score(labels, np.round(probs)));
 * [2] uint64 number of batches.                                                            */
int rk_eval_batch(const float* logits, const float* probs, const float* labels, int64_t n,
                  int32_t loss_kind, const float* extra, void* accum, void* stream);
/* Exact roc_auc_score(labels, scores) (dcn.py:237) for n <= 2^32-1: Mann-Whitney U with ties
 * credited 1/2, from a radix sort and int64 counts; *out (device double) = NaN for a NaN score or a
 * single class.  workspace: rk_auc_workspace_size(n) bytes of device memory.                      */
int rk_auc_workspace_size(int64_t n, int64_t* bytes);
int rk_auc(const float* scores, const float* labels, int64_t n, void* workspace, int64_t ws_bytes,
           double* out, void* stream);

/* ---- per-request ranking: segmented top-K and grouped AUC (ranking.hip) ----
 * Top-K order, both forms: within a request by score descending, -0.0 == +0.0, NaN below every
 * number (-inf included), ties by the lower row.  values [R, k] float (the original bits of
 * scores[indices]), indices [R, k] int64 (rows of scores), counts [R] int64 = min(k, candidates of
 * r); slots at or past counts[r] hold -inf / -1.  1 <= k <= 1024, n <= 2^32 - 2.  No allocation, no
 * synchronisation, capturable; R == 0 returns RK_OK without a launch.
 * rk_topk_segments: request r owns the contiguous rows offsets[r] .. offsets[r+1] of scores[n]
 *   (offsets non-decreasing).  One launch, one wave per request, the running best kept in
 *   registers; k <= RK_TOPK_SEGMENT_MAX_K (else RK_ERR_UNSUPPORTED: use rk_topk_segments_sorted).
 *   An offset outside [0, n] is clamped and raises RK_FLAG_INDEX_OOB: no row past n is read.
 * rk_topk_segments_sorted: the same result for every k by the sort path of rk_topk_by_request;
 *   rows that no segment covers are left out.
 * rk_topk_by_request: row b belongs to request request_index[b], in any order.  A stable radix
 *   sort of (request, inverted order-preserving score bits) with the row as value, over the bits
 *   R needs; then the first k rows of each request.  A request_index outside [0, R) is left out
 *   and raises RK_FLAG_INDEX_OOB.  workspace: rk_topk_by_request_workspace_size(n, R) bytes (for
 *   both sorted entry points).                                                                  */
#define RK_TOPK_MAX_K 1024
#define RK_TOPK_SEGMENT_MAX_K 64
int rk_topk_segments(const float* scores, int64_t n, const int64_t* offsets, int64_t R, int32_t k,
                     float* values, int64_t* indices, int64_t* counts, void* stream);
int rk_topk_by_request_workspace_size(int64_t n, int64_t R, int64_t* bytes);
int rk_topk_segments_sorted(const float* scores, int64_t n, const int64_t* offsets, int64_t R, int32_t k,
                            float* values, int64_t* indices, int64_t* counts, void* workspace,
                            int64_t ws_bytes, void* stream);
int rk_topk_by_request(const float* scores, const int64_t* request_index, int64_t n, int64_t R,
                       int32_t k, float* values, int64_t* indices, int64_t* counts, void* workspace,
                       int64_t ws_bytes, void* stream);
/* AUC per group and its impression-weighted mean (GAUC, the DIN / DIEN papers' metric), rk_auc's
 * integer scheme per group: sort by (group, score) with -0.0 == +0.0, reduce equal pairs to
 * (positives, negatives), negatives-before by a scan that restarts at each group,
 * 2U_g = sum pos (2 neg_before + neg) in int64.  Outputs, one row per group present in ascending
 * group id (arrays of n entries, the first *n_groups written): group_ids, two_u, pos, neg (int64);
 * n_groups: device int64.  summary (3 x 8 bytes): [0] double GAUC = sum_g n_g U_g / (P_g N_g) /
 * sum_g n_g over the groups with both classes, n_g = P_g + N_g, summed in a fixed order (no
 * floating atomics: the same bits for any order of the rows); NaN when no group is valid or a valid
 * group holds a NaN score; [1] int64 number of valid groups; [2] int64 their row total.  A group
 * id outside [0, 2^31) is left out and raises RK_FLAG_INDEX_OOB.  1 <= n <= 2^32 - 2.
 * workspace: rk_grouped_auc_workspace_size(n) bytes.                                            */
int rk_grouped_auc_workspace_size(int64_t n, int64_t* bytes);
int rk_grouped_auc(const float* scores, const float* labels, const int64_t* groups, int64_t n,
                   void* workspace, int64_t ws_bytes, void* summary, int64_t* group_ids, int64_t* two_u,
                   int64_t* pos, int64_t* neg, int64_t* n_groups, void* stream);

int rk_bn_fold(const float* mean, const float* var, const float* weight, const float* bias,
               float eps, int32_t n, float* scale, float* shift, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RANKOPS_H */
