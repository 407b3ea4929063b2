// ESMM (Entire Space Multi-task Model, Ma et al., SIGIR 2018) forward in one launch, on the fused-MLP
// machinery of mlp_core.h / mtl_core.h that mmoe.hip uses: 16 rows per workgroup of 16 waves, FP32 MFMA
// (v_mfma_f32_16x16x4_f32), fragment-major packed weights streamed through the 8-slot ring.
//
//   x       = the gathered row (rk_concat_gather's column map, as mlp_gather_kernel)
//   logit_k = head_k(tower_k(x))                   every tower reads the same x
//   cond_k  = sigmoid(logit_k)                     the conditional probability (pCTR, pCVR, ...)
//   prob_k  = cond_0 cond_1 ... cond_k             the entire-space probability (pCTR, pCTCVR, ...), k ascending
//
// Phases of a workgroup (a barrier after each layer; the next layer's weight ring is issued before that
// barrier, LayerPipe::prepare):
//   1. wave w gathers row m0 + w into xs (stays there: every tower's first layer reads it)
//   2. towers k = 0..K-1: layer 0 from xs, later layers ping-pong ha / hb, then the head (one wave per
//      row); its logit goes to lg[row][k] and to `logits`
//   3. one thread per row walks k ascending over lg and writes the running product (`probs`) and the
//      conditionals (`cond`)
// The row is gathered once for all towers and no tower activation reaches HBM in eval.  Every sum runs
// in a fixed order: two runs give the same bits.
//
// LDS (floats): xs [16][pad64(width) + 8], ha and hb [16][max pad64(hidden) + 8], lg [16][8].
//
// mm_view and mm_train_store have copies here (es_view, es_train_store): moved into mtl_core.h they
// would be compiled into mmoe.hip from another place, and mmoe.hip's comments record what such moves cost.
#include "mtl_core.h"
#include "train_common.h"

namespace rk {

constexpr int kEsMaxTasks = 8;
constexpr int kEsMaxDepth = 3;

struct EsmmArgs {
  RowMap map;
  rk_mmoe_layer layers[kEsMaxTasks * kEsMaxDepth];  // tower k layer l at [k Dt + l]
  const float* head_w[kEsMaxTasks];
  const float* head_b[kEsMaxTasks];
  int64_t M;
  int width, K, Dt;
  int ldx, ldh;  // LDS row strides (floats)
  float* logits;
  float* probs;
  float* cond;
  uint32_t* flags;
};
static_assert(sizeof(EsmmArgs) <= 4096, "kernel arguments beyond 4 KiB");

// The train forward's additions (rk_esmm_forward_train): dropout behind every ReLU and the buffers the
// backward reads, in rk_mmoe_forward_train's tower layout: tower k's layer l at columns k * pitch_t[l]
// of tact[l] [B, K * pitch_t[l]], a pitch the width rounded up to 4, zeros between.  Dropout site
// k Dt + l keeps element (b, j) of its [B, n] output iff dropout_keep(seed + site, *slot, b n + j, threshold).
struct EsmmTrainArgs : EsmmArgs {
  float* x_out;
  float* tact[kEsMaxDepth];
  int pitch_t[kEsMaxDepth];
  int ldx_out;
  uint32_t threshold;
  float scale;
  uint64_t seed;
  const int64_t* slot;
};
static_assert(sizeof(EsmmTrainArgs) <= 4096, "kernel arguments beyond 4 KiB");

// The rk_mlp_layer view of a compact descriptor over an input of K columns (Linear + bias + act).
__device__ __forceinline__ rk_mlp_layer es_view(const rk_mmoe_layer& d, int K) {
  rk_mlp_layer L = {};
  L.w = d.w;
  L.ldw = pad64(K);
  L.n = d.n;
  L.act = d.act == RK_ACT_RELU ? RK_ACT_RELU : RK_ACT_NONE;
  L.bias = d.bias;
  return L;
}

// A finished hidden layer in LDS (16 rows of n columns, after the layer's barrier) for the train
// forward: dropout applied in place (the next layer and the head read it), the result stored to its
// column block of the layer's HBM buffer, zeros up to the pitch.  All threads; the caller's barrier follows.
__device__ __forceinline__ void es_train_store(const EsmmTrainArgs& a, float* h, int n, int site, float* dst,
                                               int64_t ld, int pitch, int64_t m0, int rows, uint64_t stream,
                                               int tid) {
  for (int i = tid; i < kMlpRows * pitch; i += kMlpThreads) {
    const int row = i / pitch, j = i - row * pitch;
    float y = 0.f;
    if (j < n) {
      y = h[row * a.ldh + j];
      if (a.threshold) {
        y = dropout_keep(a.seed + (uint64_t)site, stream, (uint64_t)(m0 + row) * n + j, a.threshold) ? y * a.scale : 0.f;
        h[row * a.ldh + j] = y;
      }
    }
    if (row < rows) dst[(m0 + row) * ld + j] = y;
  }
}

template <bool TRAIN>
__global__ __launch_bounds__(kMlpThreads) void esmm_kernel(std::conditional_t<TRAIN, EsmmTrainArgs, EsmmArgs> a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
  const int64_t m0 = (int64_t)blockIdx.x * kMlpRows;
  const int rows = (int)min<int64_t>(kMlpRows, a.M - m0);
  float* const xs = sm;
  float* const ha = xs + kMlpRows * a.ldx;
  float* const hb = ha + kMlpRows * a.ldh;
  float* const lg = hb + kMlpRows * a.ldh;
  const int width = a.width, K = a.K, Dt = a.Dt;
  const int K0p = pad64(width);
  const bool live = wave < rows;
  const int64_t b = m0 + wave;

  // 1. the row gather (mmoe_kernel's stage, written out as there): indices first, the values after
  float v[kRowCols / 64];
  int64_t r[kRowCols / 64];
  int sg[kRowCols / 64];
#pragma unroll
  for (int i = 0; i < kRowCols / 64; ++i) {
    const int c = lane + 64 * i;
    sg[i] = live && c < width ? a.map.col_seg[c] : 255;
    r[i] = b;
    if (sg[i] != 255) {
      const rk_segment& g = a.map.segs[sg[i]];
      if (g.idx) {
        r[i] = g.idx[b * g.idx_stride];
        if (r[i] < 0 || r[i] >= g.rows) {
          flag_oob(a.flags);
          r[i] = -1;
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < kRowCols / 64; ++i) {
    v[i] = 0.f;
    if (sg[i] != 255 && r[i] >= 0) {
      const rk_segment& g = a.map.segs[sg[i]];
      v[i] = g.src[r[i] * g.src_ld + a.map.col_off[lane + 64 * i]];
    }
  }
  uint64_t stream = 0;
  if constexpr (TRAIN) {
    if (a.threshold) stream = (uint64_t)*a.slot;
#pragma unroll
    for (int i = 0; i < kRowCols / 64; ++i) {
      const int c = lane + 64 * i;
      if (live && c < a.ldx_out) a.x_out[b * a.ldx_out + c] = v[i];  // (zeros past the width)
    }
  }
  __builtin_amdgcn_sched_barrier(0);  // the gather's loads stay ahead of the weight ring

  LayerPipe pipe;
  auto tower = [&](int k, int l) { return es_view(a.layers[k * Dt + l], l ? a.layers[k * Dt + l - 1].n : width); };
  {
    const rk_mlp_layer L0 = tower(0, 0);
    mtl_prepare(pipe, L0, width, wave, lane);
  }
#pragma unroll
  for (int i = 0; i < kRowCols / 64; ++i) {
    const int c = lane + 64 * i;
    if (c < K0p) xs[wave * a.ldx + c] = v[i];  // dead rows and pad columns stage zeros
  }
  mlp_lds_barrier();

  // 2. the towers, one after another, each with its head
  for (int k = 0; k < K; ++k) {
    for (int l = 0; l < Dt; ++l) {
      const int ln = lane_now(lane);
      const rk_mlp_layer L = tower(k, l);
      const int Kp = pad64(l ? a.layers[k * Dt + l - 1].n : width);
      const float* in = l == 0 ? xs : (l & 1) ? ha : hb;
      float* out = (l & 1) ? hb : ha;
      mtl_layer(pipe, L, in, l == 0 ? a.ldx : a.ldh, out, a.ldh, Kp, wave, ln);
      if (l + 1 < Dt) {
        const rk_mlp_layer N = tower(k, l + 1);
        mtl_prepare(pipe, N, L.n, wave, ln);
      } else if (k + 1 < K) {
        const rk_mlp_layer N = tower(k + 1, 0);
        mtl_prepare(pipe, N, width, wave, ln);
      }
      close_layer();
      if constexpr (TRAIN) {
        es_train_store(a, out, L.n, k * Dt + l, a.tact[l] + k * a.pitch_t[l], (int64_t)K * a.pitch_t[l], a.pitch_t[l],
                       m0, rows, stream, tid);
        mlp_lds_barrier();
      }
    }
    const float* fin = (Dt & 1) ? ha : hb;
    const int Kh = a.layers[k * Dt + Dt - 1].n;
    const int lm = lane_now(lane);
    // (the head stays written out, as in mmoe.hip: as a function taking a.head_w[k] the runtime index
    // into the by-value argument arrays moved the argument block into scratch there)
    if (live) {  // one wave per row
      const float* hw = a.head_w[k];
      float p = 0.f;
      for (int n = lm; n < Kh; n += 64) p = __builtin_fmaf(fin[wave * a.ldh + n], hw[n], p);
      p = wave_sum(p);
      if (lm == 0) {
        const float logit = p + a.head_b[k][0];
        lg[wave * kEsMaxTasks + k] = logit;
        if (a.logits) a.logits[b * K + k] = logit;
      }
    }
    mlp_lds_barrier();  // the next tower's first layer overwrites ha; lg is complete after the last one
  }

  // 3. the chain: prob_k = prob_{k-1} sigmoid(logit_k), k ascending, one thread per row
  if (tid < rows && (a.probs || a.cond)) {
    float run = 1.f;
    for (int k = 0; k < K; ++k) {
      const float c = sigmoid_fast(lg[tid * kEsMaxTasks + k]);
      run *= c;
      if (a.cond) a.cond[(m0 + tid) * K + k] = c;
      if (a.probs) a.probs[(m0 + tid) * K + k] = run;
    }
  }
}

}  // namespace rk

using namespace rk;

namespace {

// The train entry's own arguments (null for the eval entry).
struct TrainOut {
  double p;
  uint64_t seed;
  const int64_t* slot;
  float* x_out;
  float* const* tower_acts;
};

int pad4(int v) { return (v + 3) / 4 * 4; }

int esmm_launch(const char* name, const rk_segment* segs, int32_t nseg, int32_t width, int64_t batch,
                const rk_mmoe_layer* towers, int32_t num_tasks, int32_t tower_depth, const float* const* head_w,
                const float* const* head_b, float* logits, float* probs, float* cond, const TrainOut* train,
                void* stream) {
  if (!segs || !towers || !head_w || !head_b || batch < 0 || nseg <= 0 || width <= 0 || num_tasks <= 0 ||
      tower_depth < 0)
    return fail(RK_ERR_INVALID, "%s: null pointer or negative size (batch %lld)", name, (long long)batch);
  if (!(logits || probs || cond)) return fail(RK_ERR_INVALID, "%s: no output", name);
  if (nseg > kRowSegs || width > kRowCols || num_tasks < 2 || num_tasks > kEsMaxTasks || tower_depth < 1 ||
      tower_depth > kEsMaxDepth)
    return fail(RK_ERR_UNSUPPORTED, "%s: %d segments (<= %d) over %d columns (<= %d), %d tasks (2..%d), tower depth %d "
                "(1..%d)", name, nseg, kRowSegs, width, kRowCols, num_tasks, kEsMaxTasks, tower_depth, kEsMaxDepth);
  EsmmTrainArgs a = {};
  int wide = kMlpPad;  // the widest hidden activation, padded
  for (int k = 0; k < num_tasks; ++k) {
    for (int l = 0; l < tower_depth; ++l) {
      const rk_mmoe_layer& d = towers[k * tower_depth + l];
      if (!d.w || !aligned16(d.w) || d.n <= 0)
        return fail(RK_ERR_INVALID, "%s: tower %d layer %d: weight null or misaligned, n = %d", name, k, l, d.n);
      if (d.n > kMlpMaxN || (d.act != RK_ACT_NONE && d.act != RK_ACT_RELU))
        return fail(RK_ERR_UNSUPPORTED, "%s: tower %d layer %d: n = %d (<= %d), activation %d (none / ReLU)", name, k,
                    l, d.n, kMlpMaxN, d.act);
      a.layers[k * tower_depth + l] = d;
      wide = std::max(wide, pad64(d.n));
    }
    if (!head_w[k] || !head_b[k]) return fail(RK_ERR_INVALID, "%s: head %d null", name, k);
    a.head_w[k] = head_w[k];
    a.head_b[k] = head_b[k];
  }
  if (int rc = row_map_fill(a.map, segs, nseg, width, name)) return rc;
  a.M = batch;
  a.width = width;
  a.K = num_tasks;
  a.Dt = tower_depth;
  a.ldx = pad64(width) + kMlpLdPad;
  a.ldh = wide + kMlpLdPad;
  a.logits = logits;
  a.probs = probs;
  a.cond = cond;
  const size_t shm = (size_t)kMlpRows * (a.ldx + 2 * a.ldh + kEsMaxTasks) * sizeof(float);
  if (shm > 160 * 1024) return fail(RK_ERR_UNSUPPORTED, "%s: widths need %zu B of LDS", name, shm);
  a.flags = device_flags();
  if (!a.flags) return fail(RK_ERR_RUNTIME, "%s: device not initialised (rk_init)", name);
  if (train) {
    if (!(train->p >= 0.0 && train->p < 1.0) || (train->p > 0.0 && !train->slot) || !train->x_out || !train->tower_acts)
      return fail(RK_ERR_INVALID, "%s: dropout_p outside [0, 1), or a null stream slot / saved buffer", name);
    for (int l = 0; l < tower_depth; ++l) {
      for (int k = 1; k < num_tasks; ++k)
        if (towers[k * tower_depth + l].n != towers[l].n)
          return fail(RK_ERR_INVALID, "%s: tower %d layer %d is %d wide, tower 0's %d", name, k, l,
                      towers[k * tower_depth + l].n, towers[l].n);
      if (!train->tower_acts[l] || !aligned16(train->tower_acts[l]))
        return fail(RK_ERR_INVALID, "%s: tower_acts[%d] null or misaligned", name, l);
      a.tact[l] = train->tower_acts[l];
      a.pitch_t[l] = pad4(towers[l].n);
    }
    for (int i = 0; i < num_tasks * tower_depth; ++i)
      if (a.layers[i].act != RK_ACT_RELU) return fail(RK_ERR_UNSUPPORTED, "%s: every hidden layer must be ReLU", name);
    if (!aligned16(train->x_out)) return fail(RK_ERR_INVALID, "%s: x_out misaligned", name);
    a.x_out = train->x_out;
    a.ldx_out = pad4(width);
    a.threshold = dropout_threshold(train->p);
    a.scale = (float)(1.0 / (1.0 - train->p));
    a.seed = train->seed;
    a.slot = train->slot;
  }
  if (batch == 0) return RK_OK;
  const int64_t blocks = (batch + kMlpRows - 1) / kMlpRows;
  if (blocks > INT32_MAX) return fail(RK_ERR_UNSUPPORTED, "%s: batch too large", name);
  if (train) {
    raise_lds_limit((const void*)esmm_kernel<true>, 160 * 1024);
    esmm_kernel<true><<<(unsigned)blocks, kMlpThreads, shm, (hipStream_t)stream>>>(a);
  } else {
    raise_lds_limit((const void*)esmm_kernel<false>, 160 * 1024);
    esmm_kernel<false><<<(unsigned)blocks, kMlpThreads, shm, (hipStream_t)stream>>>(static_cast<const EsmmArgs&>(a));
  }
  return check_launch(name);
}

}  // namespace

RK_API int rk_esmm_forward(const rk_segment* segs, int32_t nseg, int32_t width, int64_t batch,
                           const rk_mmoe_layer* towers, int32_t num_tasks, int32_t tower_depth,
                           const float* const* head_w, const float* const* head_b, float* logits, float* probs,
                           float* cond, void* stream) {
  return esmm_launch("rk_esmm_forward", segs, nseg, width, batch, towers, num_tasks, tower_depth, head_w, head_b, logits,
                     probs, cond, nullptr, stream);
}

RK_API int rk_esmm_forward_train(const rk_segment* segs, int32_t nseg, int32_t width, int64_t batch,
                                 const rk_mmoe_layer* towers, int32_t num_tasks, int32_t tower_depth,
                                 const float* const* head_w, const float* const* head_b, double dropout_p, uint64_t seed,
                                 const int64_t* stream_slot, float* x_out, float* const* tower_acts, float* logits,
                                 float* probs, float* cond, void* stream) {
  const TrainOut t = {dropout_p, seed, stream_slot, x_out, tower_acts};
  return esmm_launch("rk_esmm_forward_train", segs, nseg, width, batch, towers, num_tasks, tower_depth, head_w, head_b,
                     logits, probs, cond, &t, stream);
}
