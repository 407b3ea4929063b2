// The whole DIEN eval forward in one launch (rankops/dien.py DIEN.forward): per 16-sample workgroup of
// 16 waves, the row [dense | category embeddings | target embedding | final interest state] is built in
// LDS and the fcn tail + output layer + sigmoid run over it on the streamed plan (mlp_stream.h).
// Replaces rk_concat_gather + rk_dien_interest + rk_mlp_forward (three launches and the row's round
// trip through HBM); prob, logit and the attention weights are bit-equal to theirs.
//
//  * Chain waves (0-3): wave w runs samples m0 + 4w .. 4w + 3, one DPP row of 16 lanes per sample, in
//    dien_interest_kernel's lane mapping, and calls its phases (dien_cell.h) in its order, so state and
//    attention have rk_dien_interest's bits.  The query is the target row: the sample's 16 lanes gather
//    the row's q_col columns into buf0 first and dien_project_query reads them back from there.  The
//    final state goes to the row's state columns (zeros for a sample past the batch or of length 0).
//    dien_interest_kernel separates its phases with __syncthreads(), which its one-wave workgroup
//    makes wave-local; here the chain waves order their LDS traffic with dien_wave_sync (an LDS wait +
//    a wave barrier) and execute no workgroup barrier of their own.
//  * Gather waves (4-15) fill every other column of the 16 rows meanwhile (rk_concat_gather's
//    semantics: the last covering segment wins, an out-of-range id reads zero and raises the flag;
//    zeros past `width` and for rows past the batch).
//  * Then all 16 waves run mlp_stream_rows<P> over buf0 / buf1: P = StreamPlanK128, the plan
//    rk_mlp_forward picks for this tail, or StreamPlanK80 when the row fits 80 columns (layer 0 streams
//    5 of its image's 8 K chunks; the other 3 multiply zero columns, so the sums are the same).  Its
//    first workgroup barrier is the one that hands the rows over; every wave executes exactly the
//    barriers inside mlp_stream_rows (8 on either plan, the same in both of its wave classes), on
//    every path: nothing before it branches around a workgroup barrier.
//
// LDS (floats): buf0 [16][ld0] | at off1: buf1 [16][ld1], aliased by the 16 per-sample slices
// [T][max(H, nh)] rows, [pad4(T)] scores, [16] A . e_target of dien_interest_kernel (phase B writes
// buf1 only after the barrier that opens it, when every chain is done).
#include <new>

#include "dien_cell.h"
#include "mlp_stream.h"

namespace rk {

constexpr int kDfSegs = 32;
constexpr int kDfCols = 128;      // row columns within one 128-wide K plan
constexpr int kDfChainWaves = 4;  // 4 samples each: the workgroup's 16 rows
constexpr int kDfNH = 8;
static_assert(kDfChainWaves * kDienSamples == kMlpRows, "one chain per row of the tail's tile");

struct DienFwdArgs {
  rk_segment segs[kDfSegs];
  uint8_t col_seg[kDfCols], col_off[kDfCols];  // row column -> (segment, offset); 255: zero
  int width, q_col, state_col;
  const float* key_table;
  int64_t key_rows, ld_key;
  const int64_t* seq;
  int64_t ld_seq;
  int T;
  const int64_t* seq_len;
  int64_t batch;
  DienWeights w;
  int cell_type;
  float* att_out;
  int64_t ld_att;
  uint32_t* flags;
  rk_mlp_layer L[RK_MLP_MAX_LAYERS];
  rk_epilogue head;
  int ld0, ld1, off1;  // LDS (floats): buf0 [16][ld0]; at off1 buf1 [16][ld1] / the DIEN slices
  int sample_stride;   // floats per DIEN slice
};
static_assert(sizeof(DienFwdArgs) <= 4096, "kernel arguments beyond 4 KiB");

// Orders a wave's LDS traffic between two phases of a chain: what its lanes stored is visible to its
// other lanes' loads after this.
__device__ __forceinline__ void dien_wave_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// Column c of sample b's row as rk_concat_gather fills it.
__device__ __forceinline__ float dien_row_column(const DienFwdArgs& a, int64_t b, int c, bool live) {
  float v = 0.f;
  const int sg = live && c < a.width ? a.col_seg[c] : 255;
  if (sg != 255) {
    const rk_segment& g = a.segs[sg];
    int64_t r = b;
    if (g.idx) {
      r = g.idx[b * g.idx_stride];
      if (r < 0 || r >= g.rows) {
        flag_oob(a.flags);
        r = -1;
      }
    }
    if (r >= 0) v = g.src[r * g.src_ld + a.col_off[c]];
  }
  return v;
}

template <int H, class P>
__global__ __launch_bounds__(kMlpThreads) void dien_forward_kernel(DienFwdArgs a) {
  constexpr int NH = kDfNH, RW = H > NH ? H : NH;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
  const int64_t m0 = (int64_t)blockIdx.x * kMlpRows;
  const int rows = (int)min<int64_t>(kMlpRows, a.batch - m0);
  float* const buf0 = sm;
  float* const buf1 = sm + a.off1;
  if (wave < kDfChainWaves) {
    const int p = lane & 15, s = lane >> 4, r = kDienSamples * wave + s;
    const int64_t b = m0 + r;
    const bool live = r < rows;
    float* const row = buf0 + r * a.ld0;
    float* const hist = buf1 + (size_t)r * a.sample_stride;  // [T][RW]
    float* const att = hist + a.T * RW;                      // [T]: scores, then attention weights
    float* const wea = att + ((a.T + 3) & ~3);               // [NH]: A . e_target
    const int len = live ? dien_len(a.seq_len, b, a.T) : 0;
    for (int i = p; i < H; i += 16) row[a.q_col + i] = dien_row_column(a, b, a.q_col + i, live);
    dien_gather_rows<H, RW>(a.key_table, a.key_rows, a.ld_key, a.seq, a.ld_seq, 0, b, len, p, a.flags, hist);
    dien_wave_sync();
    dien_project_query<H, NH>(a.w.A, row + a.q_col, 0, b, live, p, wea);
    dien_wave_sync();
    dien_extract_pass<H, NH, RW, true, false>(a.w.Wg, a.w.bg, a.w.Wc, a.w.bc, hist, len, p, nullptr, b, a.T);
    dien_wave_sync();
    dien_attention<NH, RW>(hist, wea, att, a.T, len, p, a.att_out, a.ld_att, b, live);
    dien_wave_sync();
    dien_evolve_pass<NH, RW, false>(a.w.Vg, a.w.vg, a.w.Vc, a.w.vc, hist, att, len, p, a.cell_type, nullptr, b, a.T,
                                    row + a.state_col, 0, live);
    if (!live && p < NH) row[a.state_col + p] = 0.f;
  } else {
    constexpr int kGather = kMlpThreads - kDfChainWaves * 64;
    for (int i = tid - kDfChainWaves * 64; i < kMlpRows * kDfCols; i += kGather) {
      const int r = i / kDfCols, c = i % kDfCols;
      const bool chain = (c >= a.q_col && c < a.q_col + H) || (c >= a.state_col && c < a.state_col + NH);
      if (!chain) buf0[r * a.ld0 + c] = dien_row_column(a, m0 + r, c, r < rows);
    }
  }
  mlp_stream_rows<P, kEpiRegs>(a.L, buf0, a.ld0, buf1, a.ld1, nullptr, m0, rows, a.head, tid);
}

// A prepared launch of dien_forward_kernel: validated arguments, grid and LDS size.
struct DienFwdPlan {
  DienFwdArgs a;
  int64_t blocks;
  size_t shm;
  int H;
};

}  // namespace rk

using namespace rk;

static int dien_fwd_prepare(const rk_segment* row_segs, int32_t nseg, int32_t width, int32_t q_col,
                            int32_t state_col, const float* key_table, int64_t key_rows, int64_t ld_key,
                            const int64_t* seq, int64_t ld_seq, int32_t T, const int64_t* seq_len, int64_t batch,
                            int32_t H, int32_t nh, int32_t cell_type, const float* Wg, const float* bg,
                            const float* Wc, const float* bc, const float* A, const float* Vg, const float* vg,
                            const float* Vc, const float* vc, const rk_mlp_layer* layers, int32_t nlayers,
                            const rk_epilogue* head, float* att_out, int64_t ld_att, DienFwdPlan* plan) {
  const char* who = "rk_dien_forward";
  if (!row_segs || !key_table || !seq || !seq_len || !Wg || !bg || !Wc || !bc || !A || !Vg || !vg || !Vc || !vc ||
      !layers || !head || !head->head_w)
    return fail(RK_ERR_INVALID, "%s: null pointer", who);
  if (nseg <= 0 || width <= 0 || q_col < 0 || state_col < 0 || T <= 0 || batch < 0 || H <= 0 || nh <= 0 ||
      key_rows <= 0 || ld_seq < T || ld_key < H || (att_out && ld_att < T))
    return fail(RK_ERR_INVALID, "%s: bad shape width=%d T=%d H=%d nh=%d", who, width, T, H, nh);
  if (int rc = dien_check_cell(who, cell_type)) return rc;
  if (int rc = dien_check_envelope(who, H, nh, T)) return rc;
  if (nh != kDfNH)
    return fail(RK_ERR_UNSUPPORTED, "%s: nh=%d outside the envelope of the one-launch forward (nh = %d)", who, nh,
                kDfNH);
  if (int rc = dien_check_history_rows(who, key_table, ld_key, 0)) return rc;
  if (q_col + H > width || state_col + nh > width || (q_col < state_col + nh && state_col < q_col + H))
    return fail(RK_ERR_INVALID, "%s: query columns [%d, +%d) and state columns [%d, +%d) must lie apart in a row of %d",
                who, q_col, H, state_col, nh, width);
  if (nseg > kDfSegs || width > kDfCols)
    return fail(RK_ERR_UNSUPPORTED, "%s: %d row segments over %d columns (at most %d over %d)", who, nseg, width,
                kDfSegs, kDfCols);
  *plan = DienFwdPlan{};
  DienFwdArgs& a = plan->a;
  for (int c = 0; c < kDfCols; ++c) {  // the last covering segment wins (rk_concat_gather)
    a.col_seg[c] = 255;
    a.col_off[c] = 0;
  }
  for (int sg = 0; sg < nseg; ++sg) {
    const rk_segment& g = row_segs[sg];
    if (!g.src || g.dim <= 0 || g.out_col < 0 || g.out_col + g.dim > width || (g.idx && g.rows <= 0))
      return fail(RK_ERR_INVALID, "%s: row segment %d invalid", who, sg);
    a.segs[sg] = g;
    for (int c = g.out_col; c < g.out_col + g.dim; ++c) {
      a.col_seg[c] = (uint8_t)sg;
      a.col_off[c] = (uint8_t)(c - g.out_col);
    }
  }
  if (stream_plan_for(layers, nlayers, width) != kStreamK128)
    return fail(RK_ERR_UNSUPPORTED, "%s: the fcn tail has no compiled plan over %d columns", who, width);
  int need0 = 0, need1 = 0;
  a.head = *head;
  if (int e = mlp_validate(layers, nlayers, width, a.head, &need0, &need1, who)) return e;
  for (int l = 0; l < nlayers; ++l) a.L[l] = layers[l];
  a.width = width;
  a.q_col = q_col;
  a.state_col = state_col;
  a.key_table = key_table;
  a.key_rows = key_rows;
  a.ld_key = ld_key;
  a.seq = seq;
  a.ld_seq = ld_seq;
  a.T = T;
  a.seq_len = seq_len;
  a.batch = batch;
  a.w = DienWeights{Wg, bg, Wc, bc, A, Vg, vg, Vc, vc};
  a.cell_type = cell_type;
  a.att_out = att_out;
  a.ld_att = ld_att;
  a.ld0 = need0 + kMlpLdPad;
  a.ld1 = need1 + kMlpLdPad;
  a.off1 = kMlpRows * a.ld0;
  // floats of LDS per sample: the rows, the scores and A . e_target (dien_interest_kernel's slice)
  a.sample_stride = dien_padded_stride(T * (H > nh ? H : nh) + ((T + 3) & ~3) + 16);
  const size_t region = std::max<size_t>((size_t)kMlpRows * a.sample_stride, (size_t)kMlpRows * a.ld1);
  plan->shm = ((size_t)a.off1 + region) * sizeof(float);
  if (plan->shm > 160 * 1024 - kStreamStaticLds)
    return fail(RK_ERR_UNSUPPORTED, "%s: %zu B of LDS needed (T=%d H=%d)", who, plan->shm, T, H);
  plan->blocks = (batch + kMlpRows - 1) / kMlpRows;
  if (plan->blocks > INT32_MAX) return fail(RK_ERR_UNSUPPORTED, "%s: batch too large", who);
  plan->H = H;
  a.flags = batch > 0 ? device_flags() : nullptr;  // (an empty batch launches nothing)
  return RK_OK;
}

static int dien_fwd_launch(const DienFwdPlan& p, hipStream_t st, const char* who) {
  if (p.blocks == 0) return RK_OK;
  auto go = [&](auto kern) {
    raise_lds_limit((const void*)kern, 160 * 1024);
    kern<<<(unsigned)p.blocks, kMlpThreads, p.shm, st>>>(p.a);
  };
  // the tail's K chunks: 5 when the row fits 80 columns (the other 3 multiply zero columns), else all 8
  if (p.a.width <= StreamPlanK80::KC0 * 16) {
    switch (p.H) {
      case 8: go(dien_forward_kernel<8, StreamPlanK80>); break;
      case 16: go(dien_forward_kernel<16, StreamPlanK80>); break;
      default: go(dien_forward_kernel<32, StreamPlanK80>); break;
    }
  } else {
    switch (p.H) {
      case 8: go(dien_forward_kernel<8, StreamPlanK128>); break;
      case 16: go(dien_forward_kernel<16, StreamPlanK128>); break;
      default: go(dien_forward_kernel<32, StreamPlanK128>); break;
    }
  }
  return check_launch(who);
}

#define RK_DIEN_FWD_ARG_NAMES                                                                                      \
  row_segs, nseg, width, q_col, state_col, key_table, key_rows, ld_key, seq, ld_seq, T, seq_len, batch, H, nh,     \
      cell_type, Wg, bg, Wc, bc, A, Vg, vg, Vc, vc, layers, nlayers, head, att_out, ld_att

RK_API int rk_dien_forward(const rk_segment* row_segs, int32_t nseg, int32_t width, int32_t q_col, int32_t state_col,
                           const float* key_table, int64_t key_rows, int64_t ld_key, const int64_t* seq,
                           int64_t ld_seq, int32_t T, const int64_t* seq_len, int64_t batch, int32_t H, int32_t nh,
                           int32_t cell_type, const float* Wg, const float* bg, const float* Wc, const float* bc,
                           const float* A, const float* Vg, const float* vg, const float* Vc, const float* vc,
                           const rk_mlp_layer* layers, int32_t nlayers, const rk_epilogue* head, float* att_out,
                           int64_t ld_att, void* stream) {
  DienFwdPlan p;
  if (int e = dien_fwd_prepare(RK_DIEN_FWD_ARG_NAMES, &p)) return e;
  return dien_fwd_launch(p, (hipStream_t)stream, "rk_dien_forward");
}

RK_API int rk_dien_forward_plan(const rk_segment* row_segs, int32_t nseg, int32_t width, int32_t q_col,
                                int32_t state_col, const float* key_table, int64_t key_rows, int64_t ld_key,
                                const int64_t* seq, int64_t ld_seq, int32_t T, const int64_t* seq_len, int64_t batch,
                                int32_t H, int32_t nh, int32_t cell_type, const float* Wg, const float* bg,
                                const float* Wc, const float* bc, const float* A, const float* Vg, const float* vg,
                                const float* Vc, const float* vc, const rk_mlp_layer* layers, int32_t nlayers,
                                const rk_epilogue* head, float* att_out, int64_t ld_att, void** plan_out) {
  if (!plan_out) return fail(RK_ERR_INVALID, "rk_dien_forward_plan: null plan_out");
  *plan_out = nullptr;
  DienFwdPlan* p = new (std::nothrow) DienFwdPlan;
  if (!p) return fail(RK_ERR_RUNTIME, "rk_dien_forward_plan: out of host memory");
  if (int e = dien_fwd_prepare(RK_DIEN_FWD_ARG_NAMES, p)) {
    delete p;
    return e;
  }
  *plan_out = p;
  return RK_OK;
}

RK_API int rk_dien_plan_launch(const void* plan, void* stream) {
  if (!plan) return fail(RK_ERR_INVALID, "rk_dien_plan_launch: null plan");
  return dien_fwd_launch(*static_cast<const DienFwdPlan*>(plan), (hipStream_t)stream, "rk_dien_plan_launch");
}

RK_API void rk_dien_plan_destroy(void* plan) { delete static_cast<DienFwdPlan*>(plan); }
