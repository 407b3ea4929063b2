// PLE (Progressive Layered Extraction, Tang et al., RecSys 2020) eval forward in one launch, on the
// fused-MLP machinery of mlp_core.h as mmoe.hip uses it: 16 rows per workgroup of 16 waves, FP32
// MFMA (v_mfma_f32_16x16x4_f32), fragment-major packed weights streamed through the 8-slot ring.
//
// L extraction levels.  With x_k^{-1} = x_s^{-1} = the gathered row, level j computes
//   g_k   = softmax(gate_{j,k}(x_k^{j-1}))       ms + mc columns: task k's own experts, then the shared
//   g_s   = softmax(gate_{j,s}(x_s^{j-1}))       K ms + mc columns: every expert of the level (not at
//                                                the last level)
//   f_s   = expert_{j,s}(its owner's input)      stack s = k ms + i reads x_k, s = K ms + i reads x_s
//   x_k^j = sum_c g_k[c] f,  x_s^j = sum_c g_s[c] f     c ascending
// and logit_k = head_k(tower_k(x_k^{L-1})), prob_k = sigmoid(logit_k).
//
// Phases of a workgroup (a barrier after each layer; the next layer's weight ring is issued before
// that barrier, LayerPipe::prepare):
//   1. wave w gathers row m0 + w into input slot 0 (level 0: every expert and gate reads it)
//   2. per level, the gates: K (+ 1) small GEMMs, each on its own input, into the two gate-logit
//      buffers in turn; the softmax of gate q (maximum subtracted) is one wave's work while the
//      others run gate q + 1, its weights left transposed in gt
//   3. the level's experts s = 0 .. K ms + mc - 1, layers ping-pong ha / hb; the last layer's tiles
//      stay in registers (TileSink) and each lane adds g * z into its own elements of every mixture
//      the expert belongs to (a task's expert: that task's and the shared one; a shared expert: all
//      K + 1).  s ascends, which is the gates' column order, so two runs give the same bits.
//   4. the K + 1 mixtures (accumulator layout in mt) become the next level's row-major inputs; after
//      the last level each task's mixture goes to ha, through its tower, and the head (one wave per
//      row), as in mmoe.hip.
// Nothing between the gather and the logits reaches HBM unless reps / gates ask for it.
//
// The layer descriptors of L (K ms + mc) De + L (K + 1) + K Dt + K layers do not fit in the 4 KiB of
// kernel arguments: they are a device table of rk_mmoe_layer (pointers only are read from it; every
// width comes from the arguments the host checked).
//
// LDS (floats): xin [nx][16][ldr] (nx = K + 1 inputs, 1 when L == 1), ha and hb [16][ldh],
// gs [2][16][64 + 8], gt [GC][16] (gt[(column offset + c) 16 + row]), mt [K + 1][pad64(H)][16]
// (mt[(i pad64(H) + n) 16 + row]: every element belongs to one lane, no barrier guards it).
//
// The row's column map, the per-layer dispatch (mtl_prepare, mtl_layer, mtl_layer_tiles with its
// TileSink), lane_now, close_layer and the mix into / walk over mt (mtl_mix, mtl_unmix) are
// mtl_core.h's, shared with mmoe.hip.
//
// ple_kernel<true> is the train forward (rk_ple_forward_train), as mmoe_kernel<true>: dropout behind
// every ReLU and every buffer the backward reads written on the way.  Every hidden layer, an expert's
// last one included, goes through LDS; dropout and the HBM store run from there after the layer's
// barrier, and the lanes read their mix operands back from LDS for the same fma chain, s ascending.
#include "mtl_core.h"
#include "train_common.h"

namespace rk {

constexpr int kPlMaxLevels = 4;
constexpr int kPlMaxTasks = 8;
constexpr int kPlMaxStacks = 64;  // K ms + mc: the shared gate's columns (4 tiles)
constexpr int kPlMaxDepth = 3;
constexpr int kPlLdG = kPlMaxStacks + kMlpLdPad;

__host__ __device__ constexpr int pad4(int v) { return (v + 3) / 4 * 4; }

struct PleArgs {
  RowMap map;
  const rk_mmoe_layer* table;  // device: experts [(j NE + s) De + l], gates, towers [k Dt + l], heads
  int64_t M;
  int width, L, K, ms, mc, De, Dt, H;
  int eu[kPlMaxDepth], tu[kPlMaxDepth];
  int has_head;
  int ldr, ldh, nx;
  float* logits;
  float* probs;
  float* reps[kPlMaxLevels];
  float* gates[kPlMaxLevels];
  uint32_t* flags;
};
static_assert(sizeof(PleArgs) <= 4096, "kernel arguments beyond 4 KiB");

// The train forward's additions.  Every per-layer buffer holds the layer of all stacks (tasks) of a
// level side by side: stack s of level j, layer l at columns s * p4(n_l) of eact[j * kPlMaxDepth + l]
// [B, NE * p4(n_l)], tower k's layer l at columns k * p4(n_l) of tact[l]; the columns between a width and
// its p4 hold zeros.  reps[j] is then [B, (K + 1) * p4(H)] ([B, K * p4(H)] at the last level), mixture i at
// column i * p4(H); gates[j] keeps the eval layout.  Dropout site (j NE + s) De + l for expert s of level
// j, layer l (its index in the table), L NE De + k Dt + l for tower k layer l; element (b, c) of a site's
// [B, n] output is kept iff dropout_keep(seed + site, *slot, b n + c, threshold).
struct PleTrainArgs : PleArgs {
  float* x_out;
  float* eact[kPlMaxLevels * kPlMaxDepth];
  float* tact[kPlMaxDepth];
  int ldx_out;
  uint32_t threshold;
  float scale;
  uint64_t seed;
  const int64_t* slot;
};
static_assert(sizeof(PleTrainArgs) <= 4096, "kernel arguments beyond 4 KiB");

// A finished hidden layer in LDS (16 rows of n columns, stride ldh, after the layer's barrier) for the
// train forward: dropout applied in place (the next layer reads it), the result stored to its column
// block of the layer's HBM buffer, zeros up to the pitch.  All threads; the caller's barrier follows.
__device__ __forceinline__ void pl_train_store(float* h, int ldh, int n, uint64_t key, uint64_t stream,
                                               uint32_t threshold, float scale, float* dst, int64_t ld, int pitch,
                                               int64_t m0, int rows, int tid) {
  for (int i = tid; i < kMlpRows * pitch; i += kMlpThreads) {
    const int row = i / pitch, c = i - row * pitch;
    float y = 0.f;
    if (c < n) {
      y = h[row * ldh + c];
      if (threshold) {
        y = dropout_keep(key, stream, (uint64_t)(m0 + row) * n + c, threshold) ? y * scale : 0.f;
        h[row * ldh + c] = y;
      }
    }
    if (row < rows) dst[(m0 + row) * ld + c] = y;
  }
}

template <bool TRAIN>
__global__ __launch_bounds__(kMlpThreads) void ple_kernel(std::conditional_t<TRAIN, PleTrainArgs, PleArgs> a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
  const int64_t m0 = (int64_t)blockIdx.x * kMlpRows;
  const int rows = (int)min<int64_t>(kMlpRows, a.M - m0);
  const int width = a.width, NL = a.L, K = a.K, ms = a.ms, mc = a.mc, De = a.De, Dt = a.Dt, H = a.H;
  const int NE = K * ms + mc;             // the stacks of a level: task k's at k ms + i, the shared at K ms + i
  const int GT = ms + mc;                 // a task gate's columns
  const int GC = K * GT + NE;             // gt's columns: task gate k at k GT, the shared gate at K GT
  const int Hp = pad64(H);
  float* const xin = sm;
  float* const ha = xin + a.nx * kMlpRows * a.ldr;
  float* const hb = ha + kMlpRows * a.ldh;
  float* const gs = hb + kMlpRows * a.ldh;
  float* const gt = gs + 2 * kMlpRows * kPlLdG;
  float* const mt = gt + GC * kMlpRows;
  const int K0p = pad64(width);
  const bool live = wave < rows;
  const int64_t b = m0 + wave;
  const rk_mmoe_layer* __restrict__ const table = a.table;
  const int gate0 = NL * NE * De, tower0 = gate0 + NL * (K + 1), head0 = tower0 + K * Dt;

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
  // (selects, not a[l]: an index the compiler cannot resolve into the by-value arguments' int arrays
  // moved the whole argument block into scratch)
  auto eun = [&](int l) { return l == 0 ? a.eu[0] : l == 1 ? a.eu[1] : a.eu[2]; };
  auto tun = [&](int l) { return l == 0 ? a.tu[0] : l == 1 ? a.tu[1] : a.tu[2]; };
  auto view = [&](int idx, int n, int act) {
    rk_mlp_layer L = {};
    L.w = table[idx].w;
    L.bias = table[idx].bias;
    L.n = n;
    L.act = act;
    return L;
  };
  // level j's input width, its expert s layer l, its gate q (q == K: the shared one), tower k layer l
  auto in_width = [&](int j) { return j ? H : width; };
  auto expert = [&](int j, int s, int l) {
    rk_mlp_layer L = view((j * NE + s) * De + l, eun(l), RK_ACT_RELU);
    L.ldw = pad64(l ? eun(l - 1) : in_width(j));
    return L;
  };
  auto gate = [&](int j, int q) {
    rk_mlp_layer L = view(gate0 + j * (K + 1) + q, q < K ? GT : NE, RK_ACT_NONE);
    L.ldw = pad64(in_width(j));
    return L;
  };
  auto tower = [&](int k, int l) {
    rk_mlp_layer L = view(tower0 + k * Dt + l, tun(l), RK_ACT_RELU);
    L.ldw = pad64(l ? tun(l - 1) : H);
    return L;
  };
  // input slot of owner q (a task, or K: the shared representation) at level j
  auto input = [&](int j, int q) -> const float* { return j ? xin + q * kMlpRows * a.ldr : xin; };
  {
    const rk_mlp_layer LG = gate(0, 0);
    mtl_prepare(pipe, LG, width, wave, lane);
  }
#pragma unroll
  for (int i = 0; i < kRowCols / 64; ++i) {
    const int c = lane + 64 * i;
    if (c < K0p) xin[wave * a.ldr + c] = v[i];  // dead rows and pad columns stage zeros
  }
  mlp_lds_barrier();

  for (int j = 0; j < NL; ++j) {
    const bool last_level = j + 1 == NL;
    const int nq = last_level ? K : K + 1;  // the last level has no shared gate and no shared mixture
    const int Kin = in_width(j), Kinp = pad64(Kin);
    const int gcols = K * GT + (last_level ? 0 : NE);  // columns of this level's gate output

    // 2. the gates
    for (int q = 0; q < nq; ++q) {
      const int ln = lane_now(lane);
      const rk_mlp_layer LG = gate(j, q);
      float* const gq = gs + (q & 1) * kMlpRows * kPlLdG;
      mtl_layer(pipe, LG, input(j, q), a.ldr, gq, kPlLdG, Kinp, wave, ln);
      {  // the next gate, or the level's first expert (one prepare for both: the descriptor is chosen, not the call)
        const bool more = q + 1 < nq;
        rk_mlp_layer N = view(more ? gate0 + j * (K + 1) + q + 1 : j * NE * De, more ? (q + 1 < K ? GT : NE) : eun(0),
                              more ? RK_ACT_NONE : RK_ACT_RELU);
        N.ldw = Kinp;
        mtl_prepare(pipe, N, Kin, wave, ln);
      }
      close_layer();
      // softmax of gate q: one wave outside the four that own the next gate's tiles; lane = row + 16 part,
      // part p takes the columns c = p, p + 4, ...
      if (wave == 4 + (q & 7)) {
        const int row = ln & 15, part = ln >> 4, n = LG.n, off = q * GT;
        const float* const p = gq + row * kPlLdG;
        float mx = -INFINITY;
        for (int c = part; c < n; c += 4) mx = fmaxf(mx, p[c]);
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        float s = 0.f;
        for (int c = part; c < n; c += 4) s += expf(p[c] - mx);
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        float* const go = a.gates[j];
        for (int c = part; c < n; c += 4) {
          const float w = expf(p[c] - mx) / s;
          gt[(off + c) * kMlpRows + row] = w;
          if (go && row < rows) go[(m0 + row) * gcols + off + c] = w;
        }
      }
    }
    mlp_lds_barrier();  // the last gate's weights are in gt

    // 3. the experts; the mix after the last layer's epilogue
    for (int s = 0; s < NE; ++s) {
      const int owner = s < K * ms ? s / ms : K;
      const float* const x0 = input(j, owner);
      for (int l = 0; l < De; ++l) {
        const int ln = lane_now(lane);
        const rk_mlp_layer L = expert(j, s, l);
        const int Kp = pad64(l ? eun(l - 1) : Kin);
        const float* in = l == 0 ? x0 : (l & 1) ? ha : hb;
        float* out = (l & 1) ? hb : ha;
        // what runs next (one prepare for every case: the descriptor is chosen, not the call): this expert's
        // next layer, the next expert, the next level's first gate, or the first tower
        int nidx = (j * NE + s) * De + l + 1, nn = eun(l + 1 < De ? l + 1 : 0), nk = L.n, nact = RK_ACT_RELU;
        bool has_next = true;
        if (l + 1 == De) {
          nk = Kin;
          if (s + 1 == NE) {
            nk = H;
            if (!last_level) {
              nidx = gate0 + (j + 1) * (K + 1);
              nn = GT;
              nact = RK_ACT_NONE;
            } else {
              nidx = tower0;
              nn = tun(0);
              has_next = a.has_head && Dt > 0;
            }
          }
        }
        rk_mlp_layer N = view(has_next ? nidx : 0, nn, nact);
        N.ldw = pad64(nk);
        if (l + 1 < De) {
          mtl_layer(pipe, L, in, l == 0 ? a.ldr : a.ldh, out, a.ldh, Kp, wave, ln);
          mtl_prepare(pipe, N, nk, wave, ln);
          if constexpr (TRAIN) {
            close_layer();
            const int pitch = pad4(L.n);
            pl_train_store(out, a.ldh, L.n, a.seed + (uint64_t)((j * NE + s) * De + l), stream, a.threshold, a.scale,
                           a.eact[j * kPlMaxDepth + l] + s * pitch, (int64_t)NE * pitch, pitch, m0, rows, tid);
          }
        } else {
          // (train: the last layer goes through LDS like the others, so that dropout and the store of f_s
          // run after its barrier, as in mmoe_kernel<true>)
          f32x4_t z[2];
          if constexpr (TRAIN)
            mtl_layer(pipe, L, in, l == 0 ? a.ldr : a.ldh, out, a.ldh, Kp, wave, ln);
          else
            mtl_layer_tiles(pipe, L, in, l == 0 ? a.ldr : a.ldh, Kp, wave, ln, z);
          if (has_next) mtl_prepare(pipe, N, nk, wave, ln);
          if constexpr (TRAIN) {
            close_layer();
            const int pitch = pad4(H);
            pl_train_store(out, a.ldh, H, a.seed + (uint64_t)((j * NE + s) * De + l), stream, a.threshold, a.scale,
                           a.eact[j * kPlMaxDepth + l] + s * pitch, (int64_t)NE * pitch, pitch, m0, rows, tid);
            mlp_lds_barrier();
            const int q4 = (ln >> 4) * 4;  // the lane's first row
#pragma unroll
            for (int t = 0; t < 2; ++t) {
              const int n = 16 * (wave + kMlpWaves * t) + (ln & 15);
#pragma unroll
              for (int q = 0; q < 4; ++q) z[t][q] = n < Hp ? out[(q4 + q) * a.ldh + n] : 0.f;
            }
          }
          // mixtures i0 .. i1 - 1 take this expert (a task's expert: its task, then the shared one below)
          const int i0 = owner < K ? owner : 0, i1 = owner < K ? owner + 1 : K;
          const int col = owner < K ? s - owner * ms : ms + (s - K * ms);  // its column of a task gate
          for (int i = i0; i <= i1; ++i) {
            int slot = i, gcol = i * GT + col;
            bool first = ms > 0 ? s == i * ms : s == 0;
            if (i == i1) {  // the shared mixture, column s of the shared gate
              if (last_level) break;
              slot = K;
              gcol = K * GT + s;
              first = s == 0;
            }
            mtl_mix(mt, gt, slot, gcol, first, z, Hp, wave, ln);
          }
        }
        // (train: also the barrier pl_train_store relies on — its in-place dropout is complete before the
        // next layer reads `out`, and the mix's LDS readback before the next expert overwrites it)
        close_layer();
      }
    }

    if (!last_level) {
      // 4a. the K + 1 mixtures -> the next level's row-major inputs (pad columns hold zeros) and reps[j]
      const int lm = lane_now(lane);
      float* const ro = a.reps[j];
      for (int i = 0; i <= K; ++i) {
        float* const xi = xin + i * kMlpRows * a.ldr;
        mtl_unmix(mt, i, Hp, wave, lm, [&](int row, int n, float m) {
          xi[row * a.ldr + n] = m;
          if constexpr (TRAIN) {
            const int pm = pad4(H);
            if (n < pm && row < rows) ro[((m0 + row) * (K + 1) + i) * pm + n] = n < H ? m : 0.f;
          } else {
            if (ro && n < H && row < rows) ro[((m0 + row) * (K + 1) + i) * H + n] = m;
          }
        });
      }
      mlp_lds_barrier();
    }
  }

  // 4b. per task: the last level's mixture to LDS row-major (and reps[L - 1]), the tower, the head
  {
    float* const ro = a.reps[NL - 1];
    for (int k = 0; k < K; ++k) {
      const int lm = lane_now(lane);
      mtl_unmix(mt, k, Hp, wave, lm, [&](int row, int n, float m) {
        if (a.has_head) ha[row * a.ldh + n] = m;  // pad columns hold zeros: the tower's zero K pad
        if constexpr (TRAIN) {
          const int pm = pad4(H);
          if (n < pm && row < rows) ro[((m0 + row) * K + k) * pm + n] = n < H ? m : 0.f;
        } else {
          if (ro && n < H && row < rows) ro[((m0 + row) * K + k) * H + n] = m;
        }
      });
      if (!a.has_head) continue;
      mlp_lds_barrier();
      for (int l = 0; l < Dt; ++l) {
        const int ln = lane_now(lane);
        const rk_mlp_layer L = tower(k, l);
        const int Kp = pad64(l ? tun(l - 1) : H);
        const float* in = (l & 1) ? hb : ha;
        float* out = (l & 1) ? ha : hb;
        mtl_layer(pipe, L, in, a.ldh, out, a.ldh, Kp, wave, ln);
        if (l + 1 < Dt) {
          const rk_mlp_layer N = tower(k, l + 1);
          mtl_prepare(pipe, N, L.n, wave, ln);
        } else if (k + 1 < K) {
          const rk_mlp_layer N = tower(k + 1, 0);
          mtl_prepare(pipe, N, H, wave, ln);
        }
        close_layer();
        if constexpr (TRAIN) {
          const int pitch = pad4(L.n);
          pl_train_store(out, a.ldh, L.n, a.seed + (uint64_t)(gate0 + k * Dt + l), stream, a.threshold, a.scale,
                         a.tact[l] + k * pitch, (int64_t)K * pitch, pitch, m0, rows, tid);
          mlp_lds_barrier();
        }
      }
      const float* fin = (Dt & 1) ? hb : ha;
      const int Kh = Dt ? tun(Dt - 1) : H;
      if (live) {  // one wave per row
        const float* hw = table[head0 + k].w;
        float p = 0.f;
        for (int n = lm; n < Kh; n += 64) p = __builtin_fmaf(fin[wave * a.ldh + n], hw[n], p);
        p = wave_sum(p);
        if (lm == 0) {
          const float logit = p + table[head0 + k].bias[0];
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
  float* const* expert_acts;  // [j * expert_depth + l]
  float* const* tower_acts;
};

int ple_launch(const char* name, const rk_segment* segs, int32_t nseg, int32_t width, int64_t batch, int32_t num_levels,
               int32_t num_tasks, int32_t num_specific, int32_t num_shared, const int32_t* expert_units,
               int32_t expert_depth, const int32_t* tower_units, int32_t tower_depth, int32_t has_heads,
               const rk_mmoe_layer* table, int64_t table_len, float* logits, float* probs, float* const* level_reps,
               float* const* level_gates, const TrainOut* train, void* stream) {
  if (!segs || !table || !expert_units || batch < 0 || nseg <= 0 || width <= 0 || num_levels <= 0 || num_tasks <= 0 ||
      num_specific < 0 || num_shared <= 0 || expert_depth <= 0 || tower_depth < 0 || (tower_depth > 0 && !tower_units) ||
      (tower_depth > 0 && !has_heads))
    return fail(RK_ERR_INVALID, "%s: null pointer or negative size (batch %lld)", name, (long long)batch);
  if (!has_heads && (logits || probs)) return fail(RK_ERR_INVALID, "%s: logits / probs need the heads", name);
  const int L = num_levels, K = num_tasks, ms = num_specific, mc = num_shared, De = expert_depth, Dt = tower_depth;
  const int64_t NE = (int64_t)K * ms + mc;
  if (nseg > kRowSegs || width > kRowCols || L > kPlMaxLevels || K > kPlMaxTasks || ms > kPlMaxStacks ||
      mc > kPlMaxStacks || NE > kPlMaxStacks || De > kPlMaxDepth || Dt > kPlMaxDepth)
    return fail(RK_ERR_UNSUPPORTED, "%s: %d segments (<= %d) over %d columns (<= %d), %d levels (<= %d), %d tasks (<= %d), "
                "%d specific and %d shared experts (tasks x specific + shared <= %d) of depth %d (1..%d), tower depth %d "
                "(<= %d)", name, nseg, kRowSegs, width, kRowCols, L, kPlMaxLevels, K, kPlMaxTasks, ms, mc, kPlMaxStacks,
                De, kPlMaxDepth, Dt, kPlMaxDepth);
  bool any_out = logits || probs;
  for (int j = 0; j < L; ++j) any_out = any_out || (level_reps && level_reps[j]) || (level_gates && level_gates[j]);
  if (!any_out) return fail(RK_ERR_INVALID, "%s: no output", name);
  PleTrainArgs a = {};
  int wide = kMlpPad;  // the widest hidden activation, padded
  for (int l = 0; l < De + Dt; ++l) {
    const int n = l < De ? expert_units[l] : tower_units[l - De];
    if (n <= 0) return fail(RK_ERR_INVALID, "%s: %s layer %d: n = %d", name, l < De ? "expert" : "tower", l < De ? l : l - De, n);
    if (n > kMlpMaxN)
      return fail(RK_ERR_UNSUPPORTED, "%s: %s layer %d: n = %d (<= %d)", name, l < De ? "expert" : "tower",
                  l < De ? l : l - De, n, kMlpMaxN);
    (l < De ? a.eu[l] : a.tu[l - De]) = n;
    wide = std::max(wide, pad64(n));
  }
  const int H = expert_units[De - 1];
  const int64_t want = (int64_t)L * NE * De + (int64_t)L * (K + 1) + (has_heads ? (int64_t)K * Dt + K : 0);
  if (table_len != want || !aligned16(table) || ((uintptr_t)table & 7u))
    return fail(RK_ERR_INVALID, "%s: the layer table holds %lld descriptors, this shape needs %lld", name,
                (long long)table_len, (long long)want);
  if (int rc = row_map_fill(a.map, segs, nseg, width, name)) return rc;
  a.table = table;
  a.M = batch;
  a.width = width;
  a.L = L;
  a.K = K;
  a.ms = ms;
  a.mc = mc;
  a.De = De;
  a.Dt = Dt;
  a.H = H;
  a.has_head = has_heads != 0;
  a.nx = L > 1 ? K + 1 : 1;
  a.ldr = pad64(L > 1 ? std::max(width, H) : width) + kMlpLdPad;
  a.ldh = wide + kMlpLdPad;
  a.logits = logits;
  a.probs = probs;
  for (int j = 0; j < L; ++j) {
    a.reps[j] = level_reps ? level_reps[j] : nullptr;
    a.gates[j] = level_gates ? level_gates[j] : nullptr;
  }
  // LDS: the level inputs, the activation buffers, the gate logits and weights, the K + 1 mixtures
  const int64_t GC = (int64_t)K * (ms + mc) + NE;
  const size_t shm = (size_t)kMlpRows * ((size_t)a.nx * a.ldr + 2 * a.ldh + 2 * kPlLdG + GC + (size_t)(K + 1) * pad64(H)) *
                     sizeof(float);
  if (shm > 160 * 1024) return fail(RK_ERR_UNSUPPORTED, "%s: this shape needs %zu B of LDS (<= %d)", name, shm, 160 * 1024);
  a.flags = device_flags();
  if (!a.flags) return fail(RK_ERR_RUNTIME, "%s: device not initialised (rk_init)", name);
  if (train) {
    if (!(train->p >= 0.0 && train->p < 1.0) || (train->p > 0.0 && !train->slot) || !train->x_out || !train->expert_acts ||
        (Dt > 0 && !train->tower_acts) || !level_reps || !level_gates || (has_heads && (!logits || !probs)))
      return fail(RK_ERR_INVALID, "%s: dropout_p outside [0, 1), or a null stream slot / saved buffer", name);
    if (!aligned16(train->x_out) || !aligned16(logits) || !aligned16(probs))
      return fail(RK_ERR_INVALID, "%s: x_out / logits / probs misaligned", name);
    for (int j = 0; j < L; ++j) {
      if (!level_reps[j] || !level_gates[j] || !aligned16(level_reps[j]) || !aligned16(level_gates[j]))
        return fail(RK_ERR_INVALID, "%s: level_reps[%d] / level_gates[%d] null or misaligned", name, j, j);
      for (int l = 0; l < De; ++l) {
        float* const p = train->expert_acts[j * De + l];
        if (!p || !aligned16(p)) return fail(RK_ERR_INVALID, "%s: expert_acts[%d] null or misaligned", name, j * De + l);
        a.eact[j * kPlMaxDepth + l] = p;
      }
    }
    for (int l = 0; l < Dt; ++l) {
      if (!train->tower_acts[l] || !aligned16(train->tower_acts[l]))
        return fail(RK_ERR_INVALID, "%s: tower_acts[%d] null or misaligned", name, l);
      a.tact[l] = train->tower_acts[l];
    }
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
    raise_lds_limit((const void*)ple_kernel<true>, 160 * 1024);
    ple_kernel<true><<<(unsigned)blocks, kMlpThreads, shm, (hipStream_t)stream>>>(a);
  } else {
    raise_lds_limit((const void*)ple_kernel<false>, 160 * 1024);
    ple_kernel<false><<<(unsigned)blocks, kMlpThreads, shm, (hipStream_t)stream>>>(static_cast<const PleArgs&>(a));
  }
  return check_launch(name);
}

}  // namespace

RK_API int rk_ple_forward(const rk_segment* segs, int32_t nseg, int32_t width, int64_t batch, int32_t num_levels,
                          int32_t num_tasks, int32_t num_specific, int32_t num_shared, const int32_t* expert_units,
                          int32_t expert_depth, const int32_t* tower_units, int32_t tower_depth, int32_t has_heads,
                          const rk_mmoe_layer* table, int64_t table_len, float* logits, float* probs,
                          float* const* level_reps, float* const* level_gates, void* stream) {
  return ple_launch("rk_ple_forward", segs, nseg, width, batch, num_levels, num_tasks, num_specific, num_shared,
                    expert_units, expert_depth, tower_units, tower_depth, has_heads, table, table_len, logits, probs,
                    level_reps, level_gates, nullptr, stream);
}

RK_API int rk_ple_forward_train(const rk_segment* segs, int32_t nseg, int32_t width, int64_t batch, int32_t num_levels,
                                int32_t num_tasks, int32_t num_specific, int32_t num_shared, const int32_t* expert_units,
                                int32_t expert_depth, const int32_t* tower_units, int32_t tower_depth, int32_t has_heads,
                                const rk_mmoe_layer* table, int64_t table_len, double dropout_p, uint64_t seed,
                                const int64_t* stream_slot, float* x_out, float* const* expert_acts,
                                float* const* tower_acts, float* logits, float* probs, float* const* level_reps,
                                float* const* level_gates, void* stream) {
  const TrainOut t = {dropout_p, seed, stream_slot, x_out, expert_acts, tower_acts};
  return ple_launch("rk_ple_forward_train", segs, nseg, width, batch, num_levels, num_tasks, num_specific, num_shared,
                    expert_units, expert_depth, tower_units, tower_depth, has_heads, table, table_len, logits, probs,
                    level_reps, level_gates, &t, stream);
}
