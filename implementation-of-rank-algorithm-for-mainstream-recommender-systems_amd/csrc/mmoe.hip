// MMoE (Multi-gate Mixture-of-Experts, Ma et al., KDD 2018) eval forward in one launch, on the
// fused-MLP machinery of mlp_core.h: 16 rows per workgroup of 16 waves, FP32 MFMA
// (v_mfma_f32_16x16x4_f32), fragment-major packed weights streamed through the 8-slot ring.
//
//   x     = the gathered row (rk_concat_gather's column map, as mlp_gather_kernel)
//   g_k   = softmax_e(gate_k(x))                  one GEMM over the K stacked gates, [K E, width]
//   f_e   = expert_e(x)                           E stacks of Linear + ReLU, one after another
//   m_k   = sum_e g_k[e] f_e                      behind every expert's last layer, from its registers
//   logit_k = head_k(tower_k(m_k)),  prob_k = sigmoid(logit_k)
//
// Phases of a workgroup (a barrier after each layer; the next layer's weight ring is issued before
// that barrier, LayerPipe::prepare):
//   1. wave w gathers row m0 + w into xs (stays there: every expert's first layer reads it)
//   2. gate GEMM xs -> gs (waves 0..3 own its <= 4 column tiles), then the softmax per (row, task),
//      maximum subtracted, its weights left transposed in gt
//   3. experts e = 0..E-1: layers ping-pong ha / hb; the last layer has no LDS output: its epilogue
//      hands the wave's finished tiles back in registers (TileSink), and each lane adds
//      g[row][k][e] * z into its own elements of the per-task mixtures mt.  [B, E, H] exists
//      nowhere; e ascends, so two runs give the same bits.
//   4. per task k: the lane's mixture elements -> ha (and `mixed`), tower layers ha / hb, then the
//      head (one wave per row).
// The mixtures live in LDS, not in registers: a 16-wave workgroup has 128 VGPRs per lane, which
// mlp_layer's ring, accumulators and operands fill (mlp_gather_kernel: 126), and K x TPW x 4
// accumulators kept across the experts' layers went to scratch (240 B per lane at 4 tasks).  In mt
// every element belongs to one lane (the MFMA accumulator layout, the 4 rows of a register
// quadruple contiguous: one conflict-free 16-byte read and write per tile and task), so no barrier
// guards it.  mt holds T tasks (the host fits as many as the 160 KiB allow); with T < K steps 3 and
// 4 run once per group of T tasks.
//
// LDS (floats): xs [16][pad64(width) + 8], ha and hb [16][max pad64(hidden) + 8], gs [16][64 + 8] (the
// gate logits), gt [64][16] (the gate weights, gt[(e K + k) 16 + row]), mt [T][pad64(H)][16]
// (mt[(i pad64(H) + n) 16 + row]).
//
// The row's column map, the per-layer dispatch (mtl_prepare, mtl_layer, mtl_layer_tiles with its
// TileSink), lane_now, close_layer and the mix into / walk over mt (mtl_mix, mtl_unmix) are
// mtl_core.h's, shared with ple.hip.
#include "mtl_core.h"
#include "train_common.h"

namespace rk {

constexpr int kMmMaxExperts = 16;
constexpr int kMmMaxTasks = 8;
constexpr int kMmMaxGates = 64;  // num_tasks * num_experts: the gate GEMM's columns (4 tiles)
constexpr int kMmMaxDepth = 3;
constexpr int kMmLayers = (kMmMaxExperts + kMmMaxTasks) * kMmMaxDepth;
constexpr int kMmLdG = kMmMaxGates + kMlpLdPad;

struct MmoeArgs {
  RowMap map;
  rk_mmoe_layer layers[kMmLayers];             // expert e layer l at [e De + l], tower k layer l at [E De + k Dt + l]
  rk_mmoe_layer gate;                          // the stacked gates [K E, width]
  const float* head_w[kMmMaxTasks];
  const float* head_b[kMmMaxTasks];
  int64_t M;
  int width, E, K, De, Dt, H;
  int has_head;
  int ldx, ldh;  // LDS row strides (floats)
  int T;         // tasks mixed per pass over the experts (mt's capacity)
  float* logits;
  float* probs;
  float* mixed;
  float* gate_probs;
  uint32_t* flags;
};
static_assert(sizeof(MmoeArgs) <= 4096, "kernel arguments beyond 4 KiB");

// The train forward's additions (rk_mmoe_forward_train): dropout behind every ReLU and the buffers the
// backward reads.  Every per-layer buffer holds the layer of all experts (tasks) side by side: expert
// e's layer l at columns e * pitch_e[l] of eact[l] [B, E * pitch_e[l]], tower k's layer l at columns
// k * pitch_t[l] of tact[l] [B, K * pitch_t[l]]; a pitch is the width rounded up to 4 and the columns
// between hold zeros.  `mixed` has pitch_m floats per (row, task), x_out ldx_out per row.
// Dropout site s (expert e layer l: e De + l, tower k layer l: E De + k Dt + l) keeps element
// (b, j) of its [B, n] output iff dropout_keep(seed + s, *slot, b n + j, threshold).
struct MmoeTrainArgs : MmoeArgs {
  float* x_out;
  float* eact[kMmMaxDepth];
  float* tact[kMmMaxDepth];
  int pitch_e[kMmMaxDepth], pitch_t[kMmMaxDepth];
  int ldx_out, pitch_m;
  uint32_t threshold;
  float scale;
  uint64_t seed;
  const int64_t* slot;
};
static_assert(sizeof(MmoeTrainArgs) <= 4096, "kernel arguments beyond 4 KiB");

// The rk_mlp_layer view of a compact descriptor over an input of K columns (Linear + bias + act).
__device__ __forceinline__ rk_mlp_layer mm_view(const rk_mmoe_layer& d, int K) {
  rk_mlp_layer L = {};
  L.w = d.w;
  L.ldw = pad64(K);
  L.n = d.n;
  L.act = d.act == RK_ACT_RELU ? RK_ACT_RELU : RK_ACT_NONE;  // (the epilogue's Dice / residual variants fold away)
  L.bias = d.bias;
  return L;
}

// A finished hidden layer in LDS (16 rows of n columns, after the layer's barrier) for the train
// forward: dropout applied in place (the next layer reads it), the result stored to its column block
// of the layer's HBM buffer, zeros up to the pitch.  All threads; the caller's barrier follows.
__device__ __forceinline__ void mm_train_store(const MmoeTrainArgs& a, float* h, int n, int site, float* dst,
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
__global__ __launch_bounds__(kMlpThreads) void mmoe_kernel(std::conditional_t<TRAIN, MmoeTrainArgs, MmoeArgs> a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
  const int64_t m0 = (int64_t)blockIdx.x * kMlpRows;
  const int rows = (int)min<int64_t>(kMlpRows, a.M - m0);
  float* const xs = sm;
  float* const ha = xs + kMlpRows * a.ldx;
  float* const hb = ha + kMlpRows * a.ldh;
  float* const gs = hb + kMlpRows * a.ldh;
  float* const gt = gs + kMlpRows * kMmLdG;
  float* const mt = gt + kMlpRows * kMmMaxGates;
  const int width = a.width, E = a.E, K = a.K, De = a.De, Dt = a.Dt, H = a.H;
  const int K0p = pad64(width);
  const bool live = wave < rows;
  const int64_t b = m0 + wave;

  // 1. the row gather (mlp_gather_kernel's stage): indices first, the values after.  (Written out in each
  // of the three kernels: as one shared function it changed mlp_gather_kernel's instruction stream and
  // made mmoe_kernel slower at large batches.)
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
  auto expert = [&](int e, int l) { return mm_view(a.layers[e * De + l], l ? a.layers[e * De + l - 1].n : width); };
  auto tower = [&](int k, int l) {
    return mm_view(a.layers[E * De + k * Dt + l], l ? a.layers[E * De + k * Dt + l - 1].n : H);
  };

  // 2. the gates: one GEMM over the K stacked gate weights, then softmax over e per (row, task)
  const rk_mlp_layer LG = mm_view(a.gate, width);
  mtl_prepare(pipe, LG, width, wave, lane);
#pragma unroll
  for (int i = 0; i < kRowCols / 64; ++i) {
    const int c = lane + 64 * i;
    if (c < K0p) xs[wave * a.ldx + c] = v[i];  // dead rows and pad columns stage zeros
  }
  mlp_lds_barrier();
  mtl_layer(pipe, LG, xs, a.ldx, gs, kMmLdG, K0p, wave, lane);
  {
    const rk_mlp_layer L0 = expert(0, 0);
    mtl_prepare(pipe, L0, width, wave, lane);
  }
  close_layer();
  if (tid < kMlpRows * K) {
    const int row = tid / K, k = tid % K;
    float* const p = gs + row * kMmLdG + k * E;
    float mx = p[0];
    for (int e = 1; e < E; ++e) mx = fmaxf(mx, p[e]);
    float s = 0.f;
    for (int e = 0; e < E; ++e) {
      const float ex = expf(p[e] - mx);
      p[e] = ex;
      s += ex;
    }
    for (int e = 0; e < E; ++e) {
      const float w = p[e] / s;
      gt[(e * K + k) * kMlpRows + row] = w;
      if (a.gate_probs && row < rows) a.gate_probs[((m0 + row) * K + k) * E + e] = w;
    }
  }
  mlp_lds_barrier();

  const int Hp = pad64(H);
  for (int k0 = 0; k0 < K; k0 += a.T) {
    const int kg = min(a.T, K - k0);
    const bool more = k0 + a.T < K;  // another pass over the experts follows

    // 3. the experts; the mix after the last layer's epilogue
    for (int e = 0; e < E; ++e) {
      for (int l = 0; l < De; ++l) {
        const int ln = lane_now(lane);
        const rk_mlp_layer L = expert(e, l);
        const int Kp = pad64(l ? a.layers[e * De + l - 1].n : width);
        const float* in = l == 0 ? xs : (l & 1) ? ha : hb;
        float* out = (l & 1) ? hb : ha;
        if (l + 1 < De) {
          mtl_layer(pipe, L, in, l == 0 ? a.ldx : a.ldh, out, a.ldh, Kp, wave, ln);
          const rk_mlp_layer N = expert(e, l + 1);
          mtl_prepare(pipe, N, L.n, wave, ln);
          if constexpr (TRAIN) {
            close_layer();
            mm_train_store(a, out, L.n, e * De + l, a.eact[l] + e * a.pitch_e[l], (int64_t)E * a.pitch_e[l],
                           a.pitch_e[l], m0, rows, stream, tid);
          }
        } else {
          // (train: the last layer goes through LDS like the others, so that dropout and the store
          // of f_e run after its barrier; the register epilogue with both went to scratch)
          f32x4_t z[2];
          if constexpr (TRAIN)
            mtl_layer(pipe, L, in, l == 0 ? a.ldx : a.ldh, out, a.ldh, Kp, wave, ln);
          else
            mtl_layer_tiles(pipe, L, in, l == 0 ? a.ldx : a.ldh, Kp, wave, ln, z);
          if (e + 1 < E || (more && !(a.has_head && Dt > 0))) {
            const rk_mlp_layer N = expert(e + 1 < E ? e + 1 : 0, 0);
            mtl_prepare(pipe, N, width, wave, ln);
          } else if (a.has_head && Dt > 0) {
            const rk_mlp_layer N = tower(k0, 0);
            mtl_prepare(pipe, N, H, wave, ln);
          }
          const int q4 = (ln >> 4) * 4;  // the lane's first row
          if constexpr (TRAIN) {
            close_layer();
            mm_train_store(a, out, H, e * De + l, a.eact[l] + e * a.pitch_e[l], (int64_t)E * a.pitch_e[l],
                           a.pitch_e[l], m0, rows, stream, tid);
            mlp_lds_barrier();
#pragma unroll
            for (int j = 0; j < 2; ++j) {
              const int n = 16 * (wave + kMlpWaves * j) + (ln & 15);
#pragma unroll
              for (int q = 0; q < 4; ++q) z[j][q] = n < Hp ? out[(q4 + q) * a.ldh + n] : 0.f;
            }
          }
          for (int i = 0; i < kg; ++i) mtl_mix(mt, gt, i, e * K + k0 + i, e == 0, z, Hp, wave, ln);
        }
        close_layer();
      }
    }

    // 4. per task: the mixture to LDS row-major (and `mixed`), the tower, the head
    for (int kk = 0; kk < kg; ++kk) {
      const int k = k0 + kk;
      const int lm = lane_now(lane);
      mtl_unmix(mt, kk, Hp, wave, lm, [&](int row, int n, float m) {
        if (a.has_head) ha[row * a.ldh + n] = m;  // pad columns hold zeros: the tower's zero K pad
        if constexpr (TRAIN) {
          if (a.mixed && n < a.pitch_m && row < rows) a.mixed[((m0 + row) * K + k) * a.pitch_m + n] = n < H ? m : 0.f;
        } else {
          if (a.mixed && n < H && row < rows) a.mixed[((m0 + row) * K + k) * H + n] = m;
        }
      });
      if (!a.has_head) continue;
      mlp_lds_barrier();
      for (int l = 0; l < Dt; ++l) {
        const int ln = lane_now(lane);
        const rk_mlp_layer L = tower(k, l);
        const int Kp = pad64(l ? a.layers[E * De + k * Dt + l - 1].n : H);
        const float* in = (l & 1) ? hb : ha;
        float* out = (l & 1) ? ha : hb;
        mtl_layer(pipe, L, in, a.ldh, out, a.ldh, Kp, wave, ln);
        if (l + 1 < Dt) {
          const rk_mlp_layer N = tower(k, l + 1);
          mtl_prepare(pipe, N, L.n, wave, ln);
        } else if (kk + 1 < kg) {
          const rk_mlp_layer N = tower(k + 1, 0);
          mtl_prepare(pipe, N, H, wave, ln);
        } else if (more) {
          const rk_mlp_layer N = expert(0, 0);
          mtl_prepare(pipe, N, width, wave, ln);
        }
        close_layer();
        if constexpr (TRAIN) {
          mm_train_store(a, out, L.n, E * De + k * Dt + l, a.tact[l] + k * a.pitch_t[l], (int64_t)K * a.pitch_t[l],
                         a.pitch_t[l], m0, rows, stream, tid);
          mlp_lds_barrier();
        }
      }
      const float* fin = (Dt & 1) ? hb : ha;
      const int Kh = Dt ? a.layers[E * De + k * Dt + Dt - 1].n : H;
      // (the head stays written out here and in ple.hip: as a function taking a.head_w[k] and a.head_b[k],
      // by value or by reference, the runtime index into the by-value argument arrays moved the whole
      // argument block into scratch, 3344 B per lane)
      if (live) {  // one wave per row
        const float* hw = a.head_w[k];
        float p = 0.f;
        for (int n = lm; n < Kh; n += 64) p = __builtin_fmaf(fin[wave * a.ldh + n], hw[n], p);
        p = wave_sum(p);
        if (lm == 0) {
          const float logit = p + a.head_b[k][0];
          if (a.logits) a.logits[b * K + k] = logit;
          if (a.probs) a.probs[b * K + k] = sigmoid_fast(logit);
        }
      }
      mlp_lds_barrier();  // the next task's mixture overwrites ha
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
  float* const* expert_acts;
  float* const* tower_acts;
};

int pad4(int v) { return (v + 3) / 4 * 4; }

int mmoe_launch(const char* name, const rk_segment* segs, int32_t nseg, int32_t width, int64_t batch,
                const rk_mmoe_layer* experts, int32_t num_experts, int32_t expert_depth, const float* gate_w,
                const float* gate_b, int32_t num_tasks, const rk_mmoe_layer* towers, int32_t tower_depth,
                const float* const* head_w, const float* const* head_b, float* logits, float* probs, float* mixed,
                float* gate_probs, const TrainOut* train, void* stream) {
  if (!segs || !experts || !gate_w || batch < 0 || nseg <= 0 || width <= 0 || num_experts <= 0 || num_tasks <= 0 ||
      expert_depth <= 0 || tower_depth < 0 || (head_w != nullptr) != (head_b != nullptr) ||
      (tower_depth > 0 && (!towers || !head_w)))
    return fail(RK_ERR_INVALID, "%s: null pointer or negative size (batch %lld)", name, (long long)batch);
  if (!head_w && (logits || probs)) return fail(RK_ERR_INVALID, "%s: logits / probs need the heads", name);
  if (!(head_w ? (logits || probs || mixed || gate_probs) : (mixed || gate_probs)))
    return fail(RK_ERR_INVALID, "%s: no output", name);
  if (nseg > kRowSegs || width > kRowCols || num_experts > kMmMaxExperts || num_tasks > kMmMaxTasks ||
      num_tasks * num_experts > kMmMaxGates || expert_depth > kMmMaxDepth || tower_depth > kMmMaxDepth)
    return fail(RK_ERR_UNSUPPORTED, "%s: %d segments (<= %d) over %d columns (<= %d), %d experts (<= %d) of depth %d (1..%d), "
                "%d tasks (<= %d, tasks x experts <= %d), tower depth %d (<= %d)", name,
                nseg, kRowSegs, width, kRowCols, num_experts, kMmMaxExperts, expert_depth, kMmMaxDepth, num_tasks,
                kMmMaxTasks, kMmMaxGates, tower_depth, kMmMaxDepth);
  MmoeTrainArgs a = {};
  int wide = kMlpPad;  // the widest hidden activation, padded
  auto take = [&](const rk_mmoe_layer& d, rk_mmoe_layer& out, const char* what, int i, int l) -> int {
    if (!d.w || !aligned16(d.w) || d.n <= 0)
      return fail(RK_ERR_INVALID, "%s: %s %d layer %d: weight null or misaligned, n = %d", name, what, i, l,
                  d.n);
    if (d.n > kMlpMaxN || (d.act != RK_ACT_NONE && d.act != RK_ACT_RELU))
      return fail(RK_ERR_UNSUPPORTED, "%s: %s %d layer %d: n = %d (<= %d), activation %d (none / ReLU)", name,
                  what, i, l, d.n, kMlpMaxN, d.act);
    out = d;
    wide = std::max(wide, pad64(d.n));
    return (int)RK_OK;
  };
  for (int e = 0; e < num_experts; ++e)
    for (int l = 0; l < expert_depth; ++l)
      if (int rc = take(experts[e * expert_depth + l], a.layers[e * expert_depth + l], "expert", e, l)) return rc;
  const int H = experts[expert_depth - 1].n;
  for (int e = 1; e < num_experts; ++e)
    if (experts[e * expert_depth + expert_depth - 1].n != H)
      return fail(RK_ERR_INVALID, "%s: expert %d ends %d wide, expert 0 %d", name, e,
                  experts[e * expert_depth + expert_depth - 1].n, H);
  const int t0 = num_experts * expert_depth;
  for (int k = 0; k < num_tasks; ++k) {
    for (int l = 0; l < tower_depth; ++l)
      if (int rc = take(towers[k * tower_depth + l], a.layers[t0 + k * tower_depth + l], "tower", k, l)) return rc;
    if (head_w) {
      if (!head_w[k] || !head_b[k]) return fail(RK_ERR_INVALID, "%s: head %d null", name, k);
      a.head_w[k] = head_w[k];
      a.head_b[k] = head_b[k];
    }
  }
  if (!aligned16(gate_w)) return fail(RK_ERR_INVALID, "%s: gate image misaligned", name);
  a.gate = rk_mmoe_layer{gate_w, gate_b, num_tasks * num_experts, RK_ACT_NONE};
  if (int rc = row_map_fill(a.map, segs, nseg, width, name)) return rc;
  a.M = batch;
  a.width = width;
  a.E = num_experts;
  a.K = num_tasks;
  a.De = expert_depth;
  a.Dt = tower_depth;
  a.H = H;
  a.has_head = head_w != nullptr;
  a.ldx = pad64(width) + kMlpLdPad;
  a.ldh = wide + kMlpLdPad;
  a.logits = logits;
  a.probs = probs;
  a.mixed = mixed;
  a.gate_probs = gate_probs;
  // LDS: the activation buffers, the gates, and the mixtures of as many tasks as still fit
  const size_t base = (size_t)kMlpRows * (a.ldx + 2 * a.ldh + kMmLdG + kMmMaxGates) * sizeof(float);
  const size_t per_task = (size_t)kMlpRows * pad64(H) * sizeof(float);
  if (base + per_task > 160 * 1024)
    return fail(RK_ERR_UNSUPPORTED, "%s: widths need %zu B of LDS", name, base + per_task);
  a.T = (int)std::min<size_t>(num_tasks, (160 * 1024 - base) / per_task);
  const size_t shm = base + a.T * per_task;
  a.flags = device_flags();
  if (!a.flags) return fail(RK_ERR_RUNTIME, "%s: device not initialised (rk_init)", name);
  if (train) {
    if (!(train->p >= 0.0 && train->p < 1.0) || (train->p > 0.0 && !train->slot) || !train->x_out || !train->expert_acts ||
        (tower_depth > 0 && !train->tower_acts) || !mixed || !gate_probs)
      return fail(RK_ERR_INVALID, "%s: dropout_p outside [0, 1), or a null stream slot / saved buffer", name);
    for (int l = 0; l < expert_depth; ++l) {
      for (int e = 1; e < num_experts; ++e)
        if (experts[e * expert_depth + l].n != experts[l].n)
          return fail(RK_ERR_INVALID, "%s: expert %d layer %d is %d wide, expert 0's %d", name, e, l,
                      experts[e * expert_depth + l].n, experts[l].n);
      if (!train->expert_acts[l] || !aligned16(train->expert_acts[l]))
        return fail(RK_ERR_INVALID, "%s: expert_acts[%d] null or misaligned", name, l);
      a.eact[l] = train->expert_acts[l];
      a.pitch_e[l] = pad4(experts[l].n);
    }
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
    for (int i = 0; i < num_experts * expert_depth + num_tasks * tower_depth; ++i)
      if (a.layers[i].act != RK_ACT_RELU) return fail(RK_ERR_UNSUPPORTED, "%s: every hidden layer must be ReLU", name);
    if (!aligned16(train->x_out) || !aligned16(mixed))
      return fail(RK_ERR_INVALID, "%s: x_out / mixed misaligned", name);
    a.x_out = train->x_out;
    a.ldx_out = pad4(width);
    a.pitch_m = pad4(H);
    a.threshold = dropout_threshold(train->p);
    a.scale = (float)(1.0 / (1.0 - train->p));
    a.seed = train->seed;
    a.slot = train->slot;
  }
  if (batch == 0) return RK_OK;
  const int64_t blocks = (batch + kMlpRows - 1) / kMlpRows;
  if (blocks > INT32_MAX) return fail(RK_ERR_UNSUPPORTED, "%s: batch too large", name);
  if (train) {
    raise_lds_limit((const void*)mmoe_kernel<true>, 160 * 1024);
    mmoe_kernel<true><<<(unsigned)blocks, kMlpThreads, shm, (hipStream_t)stream>>>(a);
  } else {
    raise_lds_limit((const void*)mmoe_kernel<false>, 160 * 1024);
    mmoe_kernel<false><<<(unsigned)blocks, kMlpThreads, shm, (hipStream_t)stream>>>(static_cast<const MmoeArgs&>(a));
  }
  return check_launch(name);
}

}  // namespace

RK_API int rk_mmoe_forward(const rk_segment* segs, int32_t nseg, int32_t width, int64_t batch,
                           const rk_mmoe_layer* experts, int32_t num_experts, int32_t expert_depth,
                           const float* gate_w, const float* gate_b, int32_t num_tasks, const rk_mmoe_layer* towers,
                           int32_t tower_depth, const float* const* head_w, const float* const* head_b, float* logits,
                           float* probs, float* mixed, float* gate_probs, void* stream) {
  return mmoe_launch("rk_mmoe_forward", segs, nseg, width, batch, experts, num_experts, expert_depth, gate_w, gate_b,
                     num_tasks, towers, tower_depth, head_w, head_b, logits, probs, mixed, gate_probs, nullptr, stream);
}

RK_API int rk_mmoe_forward_train(const rk_segment* segs, int32_t nseg, int32_t width, int64_t batch,
                                 const rk_mmoe_layer* experts, int32_t num_experts, int32_t expert_depth,
                                 const float* gate_w, const float* gate_b, int32_t num_tasks,
                                 const rk_mmoe_layer* towers, int32_t tower_depth, const float* const* head_w,
                                 const float* const* head_b, double dropout_p, uint64_t seed, const int64_t* stream_slot,
                                 float* x_out, float* const* expert_acts, float* const* tower_acts, float* logits,
                                 float* probs, float* mixed, float* gate_probs, void* stream) {
  const TrainOut t = {dropout_p, seed, stream_slot, x_out, expert_acts, tower_acts};
  return mmoe_launch("rk_mmoe_forward_train", segs, nseg, width, batch, experts, num_experts, expert_depth, gate_w,
                     gate_b, num_tasks, towers, tower_depth, head_w, head_b, logits, probs, mixed, gate_probs, &t,
                     stream);
}
