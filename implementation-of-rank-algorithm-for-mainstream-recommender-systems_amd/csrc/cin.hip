// xDeepFM's Compressed Interaction Network (Lian et al. 2018, eq. 6-8, direct form) in one launch:
// the row gather, the first-order sum, every CIN layer, the pooling over d and cin_output_layer.
//
// A workgroup (8 waves) owns a tile of NC columns, column c = s * D + d for sample s of the tile
// (NC / D samples).  x0 [m][NC] and two feature-map buffers [Hmax16][NC] (layer k reads one and
// writes the other) stay in LDS; the maps never go to HBM.  Layer k is the GEMM
//   x^k[n, c] = act( sum_j W_k[n, j] * z[j, c] + bias_k[n] ),  z[h * m + i, c] = x^{k-1}[h, c] * x0[i, c]
// on v_mfma_f32_16x16x4_f32 with M = H_k, N = the tile's columns, K = H_{k-1} * m.  z is never
// stored: lane l forms its B value z[4 s + l / 16, c0 + l % 16] as one product of two LDS reads
// per K-step s, and that value feeds the wave's group of 16-row output tiles (eight at NC 128 where
// the layer has that many, else up to four).  The A operand comes from the image
// rk_cin_pack_weight writes: [row tile][K / 16][lane][4], so a lane's float4 holds its A values of
// four consecutive K-steps and a wave reads 1 KB contiguous.
// Rows past H_k and columns past K of the image are zero; a B value past K is zero too.
//
// Pooling and the logit are reduced in a fixed order (no atomics): per layer, p[s, n] = sum_d goes
// through the idle map buffer, then one wave per sample takes sum_n p[s, n] * w_out[n] (lane-strided
// partial sums, xor butterfly) and the layers are added in order.
#include "common.h"

namespace rk {
namespace {

constexpr int kCinMaxFields = 32;
constexpr int kCinMaxLayers = 4;
constexpr int kCinMaxMaps = 256;
constexpr int kCinThreads = 512;
constexpr int kCinWaves = kCinThreads / kWave;
constexpr int kCinUnitTiles = 4;  // 16-row output tiles per wave and pass over K (8 at NC 128: see the layer loop)
constexpr int kCinLdsBytes = 160 * 1024;

struct CinFields {
  const float* src2[kCinMaxFields];
  const int64_t* idx2[kCinMaxFields];
  int64_t ld2[kCinMaxFields];
  int64_t rows2[kCinMaxFields];
  int64_t istride2[kCinMaxFields];
  const float* src1[kCinMaxFields];
  const int64_t* idx1[kCinMaxFields];
  int64_t ld1[kCinMaxFields];
  int64_t rows1[kCinMaxFields];
  int64_t istride1[kCinMaxFields];
  int32_t col[kCinMaxFields];
};

struct CinLayers {
  const float* w[kCinMaxLayers];  // rk_cin_pack_weight images
  const float* bias[kCinMaxLayers];
  int32_t h[kCinMaxLayers];
};

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// One wave, NMT output tiles (rows 16 (mt0 + t) ..) of one 16-column tile: the whole K loop and the
// bias / activation epilogue into `next`.
template <int NMT>
__device__ __forceinline__ void cin_unit(const float* __restrict__ W, int KS4, int mt0, const float* prev, int hprev,
                                         const float* x0, int m, int ld, int c, int lane,
                                         const float* __restrict__ bias, int H, int act, float* next) {
  int h = 0, i = lane >> 4;
  while (i >= m) {
    i -= m;
    ++h;
  }
  f32x4 acc[NMT];
#pragma unroll
  for (int t = 0; t < NMT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const f32x4* wp = reinterpret_cast<const f32x4*>(W) + (int64_t)mt0 * KS4 * kWave + lane;
  const int64_t tstride = (int64_t)KS4 * kWave;
  // The two LDS values of the next four K-steps (h, i advance by 4 per step; m >= 2: at most two
  // wraps).  A step past K reads row 0 and is zeroed by its flag.
  float xr[4], x0r[4];
  bool ok[4];
  auto read_b = [&]() {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      ok[e] = h < hprev;
      xr[e] = prev[(ok[e] ? h : 0) * ld + c];
      x0r[e] = x0[i * ld + c];
      i += 4;
      if (i >= m) {
        i -= m;
        ++h;
      }
      if (i >= m) {
        i -= m;
        ++h;
      }
    }
  };
  f32x4 a[NMT];
#pragma unroll
  for (int t = 0; t < NMT; ++t) a[t] = wp[t * tstride];
  read_b();
  float bv[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) bv[e] = ok[e] ? xr[e] * x0r[e] : 0.f;
  for (int ks4 = 0; ks4 < KS4; ++ks4) {
    // the next 16 K: weights and LDS values in flight under this step's MFMAs (the scheduling
    // barriers keep their first uses, and so the waits, behind the MFMA block)
    f32x4 an[NMT];
    const int nx = ks4 + 1 < KS4 ? ks4 + 1 : ks4;
#pragma unroll
    for (int t = 0; t < NMT; ++t) an[t] = wp[t * tstride + (int64_t)nx * kWave];
    read_b();
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
#pragma unroll
      for (int t = 0; t < NMT; ++t) acc[t] = mfma16(a[t][e], bv[e], acc[t]);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int e = 0; e < 4; ++e) bv[e] = ok[e] ? xr[e] * x0r[e] : 0.f;
#pragma unroll
    for (int t = 0; t < NMT; ++t) a[t] = an[t];
  }
#pragma unroll
  for (int t = 0; t < NMT; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = (mt0 + t) * 16 + 4 * (lane >> 4) + r;
      if (n < H) {
        float v = acc[t][r] + (bias ? bias[n] : 0.f);
        if (act == RK_ACT_RELU) v = fmaxf(v, 0.f);
        next[n * ld + c] = v;
      }
    }
  }
}

// TRAIN: every layer's maps also go to HBM for the backward (cin_backward.hip), as
// maps[b][off_k + n][d] (sample stride hsum * D); the eval instantiation has none of that code.
template <int NC, bool TRAIN>
__global__ __launch_bounds__(kCinThreads) void cin_forward_kernel(
    const CinFields f, const CinLayers L, int m, int D, int nlayers, int act, int ld, int hp_max, int64_t batch,
    const float* __restrict__ out_w, const float* __restrict__ out_b, float* __restrict__ deep_in, int64_t ld_deep,
    float* __restrict__ fm1, float* __restrict__ pooled, int64_t ld_pooled, float* __restrict__ cin_logit,
    uint32_t* flags, float* __restrict__ maps, int hsum) {
  extern __shared__ __attribute__((aligned(16))) float cin_smem[];
  constexpr int NQ = NC / 4;   // float4 columns of the tile
  constexpr int NT = NC / 16;  // 16-column MFMA tiles
  float* x0 = cin_smem;                // [m][ld]
  float* bufA = x0 + m * ld;           // [hp_max][ld]
  float* bufB = bufA + hp_max * ld;    // [hp_max][ld]
  float* logit_l = bufB + hp_max * ld;  // [32]
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
  const int G = D >> 2;  // float4s per embedding row
  const int S = NC / D;  // samples of the tile
  const int64_t b0 = (int64_t)blockIdx.x * S;

  // ---- gather: x0[i][s D + d] (zero past the batch and for out-of-range ids), deep_in
  for (int it = tid; it < m * NQ; it += kCinThreads) {
    const int c4 = it % NQ, i = it / NQ;
    const int s = c4 / G, d0 = (c4 - s * G) * 4;
    const int64_t b = b0 + s;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (b < batch) {
      const float* row;
      if (f.idx2[i]) {
        const int64_t r = f.idx2[i][b * f.istride2[i]];
        if (r < 0 || r >= f.rows2[i]) {
          flag_oob(flags);
          row = nullptr;
        } else {
          row = f.src2[i] + r * f.ld2[i];
        }
      } else {
        row = f.src2[i] + b * f.ld2[i];
      }
      if (row) v = *reinterpret_cast<const f32x4*>(row + d0);
      if (deep_in) *reinterpret_cast<f32x4*>(deep_in + b * ld_deep + f.col[i] + d0) = v;
    }
    *reinterpret_cast<f32x4*>(x0 + i * ld + c4 * 4) = v;
  }
  // ---- first-order sum, fields in order
  if (fm1 && tid < S && b0 + tid < batch) {
    const int64_t b = b0 + tid;
    float a = 0.f;
    for (int i = 0; i < m; ++i) {
      if (f.idx1[i]) {
        const int64_t r = f.idx1[i][b * f.istride1[i]];
        if (r < 0 || r >= f.rows1[i])
          flag_oob(flags);
        else
          a += f.src1[i][r * f.ld1[i]];
      } else {
        a += f.src1[i][b * f.ld1[i]];
      }
    }
    fm1[b] = a;
  }
  if (tid < 32) logit_l[tid] = 0.f;
  __syncthreads();

  const float* prev = x0;
  int hprev = m, off = 0;
  for (int k = 0; k < nlayers; ++k) {
    const int H = L.h[k], MT = (H + 15) >> 4, Hp = MT * 16;
    const int KS4 = (hprev * m + 15) >> 4;
    float* next = (k & 1) ? bufB : bufA;
    float* idle = (k & 1) ? bufA : bufB;  // not written by this layer; free once its GEMM is done
    // units of work: (group of 16-row tiles) x (16-column tile).  With 8 column tiles (NC 128) a
    // wave takes eight row tiles at a time where there are that many (one B value for eight MFMAs,
    // one pass over K at 128 maps); the rest, and NC 64 (4 column tiles: all 8 waves stay busy at
    // 128 maps), go four at a time.
    const int g8 = NC == 128 ? MT / 8 : 0;
    const int units = (g8 + (MT - 8 * g8 + kCinUnitTiles - 1) / kCinUnitTiles) * NT;
    for (int u = wave; u < units; u += kCinWaves) {
      const int nt = u % NT, g = u / NT;
      const int c = nt * 16 + (lane & 15);
      if (g < g8) {
        cin_unit<8>(L.w[k], KS4, 8 * g, prev, hprev, x0, m, ld, c, lane, L.bias[k], H, act, next);
        continue;
      }
      const int mt0 = 8 * g8 + (g - g8) * kCinUnitTiles;
      switch (min(kCinUnitTiles, MT - mt0)) {
        case 1: cin_unit<1>(L.w[k], KS4, mt0, prev, hprev, x0, m, ld, c, lane, L.bias[k], H, act, next); break;
        case 2: cin_unit<2>(L.w[k], KS4, mt0, prev, hprev, x0, m, ld, c, lane, L.bias[k], H, act, next); break;
        case 3: cin_unit<3>(L.w[k], KS4, mt0, prev, hprev, x0, m, ld, c, lane, L.bias[k], H, act, next); break;
        default: cin_unit<4>(L.w[k], KS4, mt0, prev, hprev, x0, m, ld, c, lane, L.bias[k], H, act, next); break;
      }
    }
    __syncthreads();
    // ---- p[s][n] = sum_d x^k[n][s D + d]: four d per lane, then the G lanes of a sample
    const int total = H * NQ;
    for (int base = 0; base < total; base += kCinThreads) {
      const int id = base + tid;
      const bool ok = id < total;
      const int c4 = id % NQ, n = id / NQ;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (ok) v = *reinterpret_cast<const f32x4*>(next + n * ld + c4 * 4);
      if constexpr (TRAIN) {
        const int64_t b = b0 + c4 / G;
        if (ok && b < batch)
          *reinterpret_cast<f32x4*>(maps + ((b * hsum + off + n) * D + (c4 & (G - 1)) * 4)) = v;
      }
      float sum = (v[0] + v[1]) + (v[2] + v[3]);
      for (int o = 1; o < G; o <<= 1) sum += __shfl_xor(sum, o, kWave);
      if (ok && (c4 & (G - 1)) == 0) idle[(c4 / G) * Hp + n] = sum;
    }
    __syncthreads();
    // ---- pooled rows out; the layer's share of the logit, one wave per sample
    for (int s = wave; s < S; s += kCinWaves) {
      const int64_t b = b0 + s;
      if (b >= batch) break;
      float part = 0.f;
      for (int n = lane; n < H; n += kWave) {
        const float p = idle[s * Hp + n];
        if (pooled) pooled[b * ld_pooled + off + n] = p;
        if (cin_logit) part = fmaf(p, out_w[off + n], part);
      }
      if (cin_logit) {
        part = wave_sum(part);
        if (lane == 0) logit_l[s] += part;
      }
    }
    __syncthreads();
    prev = next;
    hprev = H;
    off += H;
  }
  if (cin_logit && nlayers > 0 && tid < S && b0 + tid < batch) cin_logit[b0 + tid] = logit_l[tid] + out_b[0];
}

__global__ __launch_bounds__(256) void cin_pack_weight_kernel(const float* __restrict__ w, int64_t ldw, int n, int k,
                                                              int KS4, int64_t total, float* __restrict__ out) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= total) return;
  const int e = (int)(o & 3), lane = (int)((o >> 2) & 63);
  const int64_t blk = o >> 8;  // mt * KS4 + ks4
  const int ks4 = (int)(blk % KS4), mt = (int)(blk / KS4);
  const int row = mt * 16 + (lane & 15), col = ks4 * 16 + e * 4 + (lane >> 4);
  out[o] = (row < n && col < k) ? w[row * ldw + col] : 0.f;
}

}  // namespace
}  // namespace rk

using namespace rk;

RK_API int rk_cin_pack_weight(const float* w, int64_t ldw, int32_t n, int32_t k, float* out, void* stream) {
  if (!w || !out || n <= 0 || k <= 0 || ldw < k || !aligned16(out))
    return fail(RK_ERR_INVALID, "rk_cin_pack_weight: bad arguments (n=%d k=%d ldw=%lld)", n, k, (long long)ldw);
  const int KS4 = (k + 15) / 16;
  const int64_t total = (int64_t)((n + 15) / 16) * KS4 * 256;
  const int64_t blocks = (total + 255) / 256;
  if (blocks > INT32_MAX) return fail(RK_ERR_UNSUPPORTED, "rk_cin_pack_weight: weight too large");
  cin_pack_weight_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(w, ldw, n, k, KS4, total, out);
  return check_launch("rk_cin_pack_weight");
}

// rk_cin_forward (maps == nullptr, the eval kernels) and rk_cin_forward_train (the TRAIN kernels)
static int cin_forward_launch(const rk_segment* second_order, const rk_segment* first_order, int32_t num_fields,
                              int32_t dim, int64_t batch, const float* const* weights, const float* const* biases,
                              const int32_t* layer_sizes, int32_t num_layers, int32_t activation, const float* out_w,
                              const float* out_b, float* deep_in, int64_t ld_deep, float* fm1, float* pooled,
                              int64_t ld_pooled, float* cin_logit, float* maps, void* stream) {
  if (!second_order || !weights || !biases || !layer_sizes || num_fields <= 0 || num_layers <= 0 || dim <= 0)
    return fail(RK_ERR_INVALID, "rk_cin_forward: null segments / layers or a non-positive count");
  if (num_fields < 2 || num_fields > kCinMaxFields)
    return fail(RK_ERR_UNSUPPORTED, "rk_cin_forward: %d fields outside [2, %d]", num_fields, kCinMaxFields);
  if (dim != 4 && dim != 8 && dim != 16 && dim != 32 && dim != 64)
    return fail(RK_ERR_UNSUPPORTED, "rk_cin_forward: dim %d not in {4, 8, 16, 32, 64}", dim);
  if (num_layers > kCinMaxLayers)
    return fail(RK_ERR_UNSUPPORTED, "rk_cin_forward: %d layers (max %d)", num_layers, kCinMaxLayers);
  if (activation != RK_ACT_NONE && activation != RK_ACT_RELU)
    return fail(RK_ERR_UNSUPPORTED, "rk_cin_forward: activation %d (identity or ReLU)", activation);
  CinLayers L;
  int hmax = 0, hsum = 0;
  for (int k = 0; k < kCinMaxLayers; ++k) {
    L.w[k] = nullptr;
    L.bias[k] = nullptr;
    L.h[k] = 0;
  }
  for (int k = 0; k < num_layers; ++k) {
    const int h = layer_sizes[k];
    if (h <= 0) return fail(RK_ERR_INVALID, "rk_cin_forward: layer %d has %d maps", k, h);
    if (h > kCinMaxMaps) return fail(RK_ERR_UNSUPPORTED, "rk_cin_forward: layer %d has %d maps (max %d)", k, h, kCinMaxMaps);
    if (!weights[k] || !aligned16(weights[k])) return fail(RK_ERR_INVALID, "rk_cin_forward: layer %d weight image", k);
    L.w[k] = weights[k];
    L.bias[k] = biases[k];
    L.h[k] = h;
    hmax = std::max(hmax, h);
    hsum += h;
  }
  if (batch < 0) return fail(RK_ERR_INVALID, "rk_cin_forward: negative batch");
  if ((fm1 && !first_order) || (cin_logit && (!out_w || !out_b)))
    return fail(RK_ERR_INVALID, "rk_cin_forward: fm1 needs first_order, cin_logit needs out_w and out_b");
  if (deep_in && (ld_deep % 4 != 0 || !aligned16(deep_in)))
    return fail(RK_ERR_INVALID, "rk_cin_forward: deep_in must be 16-B aligned with ld %% 4 == 0");
  if (pooled && ld_pooled < hsum) return fail(RK_ERR_INVALID, "rk_cin_forward: ld_pooled %lld < %d", (long long)ld_pooled, hsum);
  CinFields t;
  int dense = 0;
  for (int i = 0; i < num_fields; ++i) {
    const rk_segment& s = second_order[i];
    if (!s.src || s.dim != dim || s.out_col < 0 || s.out_col % 4 || s.src_ld % 4 || !aligned16(s.src) ||
        (s.idx && s.rows <= 0) || (deep_in && s.out_col + dim > ld_deep))
      return fail(RK_ERR_INVALID, "rk_cin_forward: field %d layout (dim %d, 16-B aligned rows)", i, dim);
    dense += s.idx == nullptr;
    t.src2[i] = s.src;
    t.idx2[i] = s.idx;
    t.ld2[i] = s.src_ld;
    t.rows2[i] = s.rows;
    t.istride2[i] = s.idx_stride;
    t.col[i] = s.out_col;
    t.src1[i] = nullptr;
    t.idx1[i] = nullptr;
    t.ld1[i] = t.rows1[i] = t.istride1[i] = 0;
    if (fm1) {
      const rk_segment& w = first_order[i];
      if (!w.src || w.dim != 1 || (w.idx && w.rows <= 0) || (w.idx == nullptr) != (s.idx == nullptr))
        return fail(RK_ERR_INVALID, "rk_cin_forward: first-order field %d", i);
      t.src1[i] = w.src;
      t.idx1[i] = w.idx;
      t.ld1[i] = w.src_ld;
      t.rows1[i] = w.rows;
      t.istride1[i] = w.idx_stride;
    }
  }
  if (dense != 0 && dense != num_fields)
    return fail(RK_ERR_UNSUPPORTED, "rk_cin_forward: segments must be all tables or all dense");
  if (batch == 0) return RK_OK;
  const bool layers = pooled || cin_logit || maps;
  if (!layers && !deep_in && !fm1) return RK_OK;
  // tile: 128 columns with rows padded by 16 floats (the four K rows of a B read on distinct banks),
  // else 64 columns, unpadded when the widest envelope (256 maps, 32 fields) needs it
  const int hp = (hmax + 15) / 16 * 16;
  auto bytes = [&](int nc, int pad) { return ((int64_t)(2 * hp + num_fields) * (nc + pad) + 32) * 4; };
  int nc = 128, pad = 16;
  if (batch * dim <= 64 || bytes(nc, pad) > kCinLdsBytes) nc = 64;
  if (bytes(nc, pad) > kCinLdsBytes) pad = 0;
  if (bytes(nc, pad) > kCinLdsBytes) return fail(RK_ERR_UNSUPPORTED, "rk_cin_forward: LDS budget");
  const int S = nc / dim;
  const int64_t blocks = (batch + S - 1) / S;
  if (blocks > INT32_MAX) return fail(RK_ERR_UNSUPPORTED, "rk_cin_forward: batch too large");
  const int lds = (int)bytes(nc, pad);
  hipStream_t st = (hipStream_t)stream;
  const int nl = layers ? num_layers : 0;
#define RK_CIN_LAUNCH(NC, TRAIN)                                                                              \
  do {                                                                                                        \
    raise_lds_limit((const void*)cin_forward_kernel<NC, TRAIN>, lds);                                         \
    cin_forward_kernel<NC, TRAIN><<<(unsigned)blocks, kCinThreads, lds, st>>>(                                \
        t, L, num_fields, dim, nl, activation, nc + pad, hp, batch, out_w, out_b, deep_in, ld_deep, fm1, pooled, \
        ld_pooled, cin_logit, device_flags(), maps, hsum);                                                    \
  } while (0)
  if (nc == 128) {
    if (maps) RK_CIN_LAUNCH(128, true);
    else RK_CIN_LAUNCH(128, false);
  } else {
    if (maps) RK_CIN_LAUNCH(64, true);
    else RK_CIN_LAUNCH(64, false);
  }
#undef RK_CIN_LAUNCH
  return check_launch(maps ? "rk_cin_forward_train" : "rk_cin_forward");
}

RK_API int rk_cin_forward(const rk_segment* second_order, const rk_segment* first_order, int32_t num_fields,
                          int32_t dim, int64_t batch, const float* const* weights, const float* const* biases,
                          const int32_t* layer_sizes, int32_t num_layers, int32_t activation, const float* out_w,
                          const float* out_b, float* deep_in, int64_t ld_deep, float* fm1, float* pooled,
                          int64_t ld_pooled, float* cin_logit, void* stream) {
  return cin_forward_launch(second_order, first_order, num_fields, dim, batch, weights, biases, layer_sizes,
                            num_layers, activation, out_w, out_b, deep_in, ld_deep, fm1, pooled, ld_pooled, cin_logit,
                            nullptr, stream);
}

RK_API int rk_cin_forward_train(const rk_segment* second_order, const rk_segment* first_order, int32_t num_fields,
                                int32_t dim, int64_t batch, const float* const* weights, const float* const* biases,
                                const int32_t* layer_sizes, int32_t num_layers, int32_t activation,
                                const float* out_w, const float* out_b, float* deep_in, int64_t ld_deep, float* fm1,
                                float* pooled, int64_t ld_pooled, float* cin_logit, float* maps, void* stream) {
  if (!maps || !aligned16(maps)) return fail(RK_ERR_INVALID, "rk_cin_forward_train: maps must be a 16-B aligned buffer");
  return cin_forward_launch(second_order, first_order, num_fields, dim, batch, weights, biases, layer_sizes,
                            num_layers, activation, out_w, out_b, deep_in, ld_deep, fm1, pooled, ld_pooled, cin_logit,
                            maps, stream);
}
