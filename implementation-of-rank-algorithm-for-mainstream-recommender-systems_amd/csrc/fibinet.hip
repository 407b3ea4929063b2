// FiBiNET (Huang et al., RecSys 2019): SENET field attention and the bilinear interaction, as its own
// launch (rk_fibinet_interaction) and as the stage of the whole eval forward in one launch
// (rk_fibinet_forward) on the fused-MLP machinery of mlp_core.h (16 rows per workgroup of 16 waves,
// FP32 MFMA, packed weights through the 8-slot ring: mlp_rows / LayerPipe).
//
//   z[s, i]    = mean_d e[s, i, d]
//   a[s, :]    = relu(W2 relu(W1 z[s, :]))
//   v[s, i, :] = a[s, i] e[s, i, :]
//   p[s, p, :] = (We e[s, i, :]) * e[s, j, :]        pair p = (i, j), i < j, lexicographic
//   q[s, p, :] = (Wv v[s, i, :]) * v[s, j, :]
//   c[s, :]    = [p[s].flatten(), q[s].flatten()]
// We / Wv: matrix 0 (type "all"), matrix i ("each") or matrix p ("interaction") of the stacked
// [nmat, D, D] weights.
//
// The interaction of a tile of S samples is one function for both kernels (fibi_interact); all of it
// runs on the VALU out of LDS, fp32, every sum in a fixed order (k ascending, one fmaf chain per
// output), no atomics: two runs give the same bits.
//   1. z: one thread per (s, i); the hidden SENET layer: one thread per (s, r); a: one thread per (s, i)
//   2. "all" / "each": u[s, i, :] = We e[s, i, :] and uv[s, i, :] = Wv v[s, i, :] for the left fields
//      i < m - 1, one thread per (i, d) holding its weight row's float4 for the S samples (every weight
//      is read once per tile), into LDS; then c's elements are products of two LDS values.
//      "interaction": one thread per (p, d), the two products stay in registers and go straight into c.
//
// LDS of a tile (floats): es [S][m D] the rows, us and uv [S][(m - 1) D] ("all" / "each" only),
// zs, hs, at [S][32] each.  rk_fibinet_forward adds mlp_rows' two activation buffers in front (c is
// written straight into the first, the MLP's input row) and lin [16] behind.
//
// The head of rk_fibinet_forward (deep_output_layer, final_layer over [linear, deep], the sigmoid) is
// written out here: mlp_rows' own head is DeepFM's three-term combine and stays as it is.
#include "mtl_core.h"

namespace rk {
namespace {

constexpr int kFibiMaxFields = 32;
constexpr int kFibiMaxDim = 64;
constexpr int kFibiMaxReduced = 32;
constexpr int kFibiThreads = 256;  // rk_fibinet_interaction's workgroup
constexpr int kFibiLdsBytes = 160 * 1024;

struct FibiFields {
  const float* src2[kFibiMaxFields];
  const int64_t* idx2[kFibiMaxFields];
  int64_t ld2[kFibiMaxFields];
  int64_t rows2[kFibiMaxFields];
  int64_t istride2[kFibiMaxFields];
  const float* src1[kFibiMaxFields];
  const int64_t* idx1[kFibiMaxFields];
  int64_t ld1[kFibiMaxFields];
  int64_t rows1[kFibiMaxFields];
  int64_t istride1[kFibiMaxFields];
};

struct FibiWeights {
  const float* w1;  // [r, m]
  const float* w2;  // [m, r]
  const float* be;  // [nmat, D, D]
  const float* bv;  // [nmat, D, D]
  int m, D, r, type;
};

// Floats of LDS a tile of S samples needs behind the caller's own buffers.
__host__ __device__ constexpr int fibi_tile_floats(int S, int m, int D, int type) {
  return S * m * D + (type == RK_FIBINET_INTERACTION ? 0 : 2 * S * (m - 1) * D) + 3 * S * kFibiMaxReduced;
}

// Four values of field i's row for sample b: zeros past the batch; an out-of-range id is flagged and reads zeros.
__device__ __forceinline__ f32x4 fibi_row4(const FibiFields& f, int i, int64_t b, int64_t batch, int d0,
                                           uint32_t* flags) {
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
  }
  return v;
}

// The first-order sum of sample b, fields in order.
__device__ __forceinline__ float fibi_first_order(const FibiFields& f, int m, int64_t b, uint32_t* flags) {
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
  return a;
}

// SENET and both bilinear layers of the S samples staged in es [S][m D] (zero rows past the batch),
// by NT threads; the caller's barrier stands between the staging and this call.  c goes to
// out[s * ldo + column] for s < srows (LDS or global), the attention to attn[s * ld_attn + i] for
// s < srows when attn is given.  Ends without a barrier: the caller's follows.
template <int S, int NT>
__device__ __forceinline__ void fibi_interact(const FibiWeights& w, const float* es, float* us, float* uv, float* zs,
                                              float* hs, float* at, float* out, int64_t ldo, int srows, float* attn,
                                              int64_t ld_attn, int tid) {
  const int m = w.m, D = w.D, r = w.r, type = w.type;
  const int lde = m * D, ldu = (m - 1) * D, G = D >> 2;
  constexpr int kA = kFibiMaxReduced;
  // ---- 1. squeeze, excitation
  for (int it = tid; it < S * m; it += NT) {
    const int s = it / m, i = it - s * m;
    const float* e = es + s * lde + i * D;
    float acc = 0.f;
    for (int d = 0; d < D; ++d) acc += e[d];
    zs[s * kA + i] = acc / (float)D;
  }
  mlp_lds_barrier();
  for (int it = tid; it < S * r; it += NT) {
    const int s = it / r, k = it - s * r;
    float acc = 0.f;
    for (int i = 0; i < m; ++i) acc = __builtin_fmaf(w.w1[k * m + i], zs[s * kA + i], acc);
    hs[s * kA + k] = fmaxf(acc, 0.f);
  }
  mlp_lds_barrier();
  for (int it = tid; it < S * m; it += NT) {
    const int s = it / m, i = it - s * m;
    float acc = 0.f;
    for (int k = 0; k < r; ++k) acc = __builtin_fmaf(w.w2[i * r + k], hs[s * kA + k], acc);
    acc = fmaxf(acc, 0.f);
    at[s * kA + i] = acc;
    if (attn && s < srows) attn[s * ld_attn + i] = acc;
  }
  mlp_lds_barrier();

  // ---- 2. the bilinear layers.  One output row d of one matrix over field i for SC samples from s0:
  // pe[s] = sum_k We[d, k] e[s, i, k], pv[s] = sum_k Wv[d, k] (a[s, i] e[s, i, k]), k ascending.
  // (SC = 8 of the 16: with all 16 in registers beside mlp_rows' weight ring the forward kernel spilled.)
  constexpr int SC = S < 8 ? S : 8;
  auto dots = [&](int mat, int i, int d, int s0, float (&pe)[SC], float (&pv)[SC]) {
    const f32x4* we = reinterpret_cast<const f32x4*>(w.be + ((int64_t)mat * D + d) * D);
    const f32x4* wv = reinterpret_cast<const f32x4*>(w.bv + ((int64_t)mat * D + d) * D);
    const float* e0 = es + s0 * lde + i * D;
#pragma unroll
    for (int s = 0; s < SC; ++s) pe[s] = pv[s] = 0.f;
#pragma unroll 1
    for (int g = 0; g < G; ++g) {
      const f32x4 a = we[g], b = wv[g];
#pragma unroll
      for (int s = 0; s < SC; ++s) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(e0 + s * lde + 4 * g);
        const float ai = at[(s0 + s) * kA + i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          pe[s] = __builtin_fmaf(a[e], x[e], pe[s]);
          pv[s] = __builtin_fmaf(b[e], ai * x[e], pv[s]);
        }
      }
    }
  };
  const int P = m * (m - 1) / 2;
  float pe[SC], pv[SC];
  if (type != RK_FIBINET_INTERACTION) {
    for (int it = tid; it < ldu; it += NT) {
      const int i = it / D, d = it - i * D;
#pragma unroll 1
      for (int s0 = 0; s0 < S; s0 += SC) {
        dots(type == RK_FIBINET_EACH ? i : 0, i, d, s0, pe, pv);
#pragma unroll
        for (int s = 0; s < SC; ++s) {
          us[(s0 + s) * ldu + it] = pe[s];
          uv[(s0 + s) * ldu + it] = pv[s];
        }
      }
    }
    mlp_lds_barrier();
  }
  for (int it = tid; it < P * D; it += NT) {
    const int p = it / D, d = it - p * D;
    int i = 0, j = p;  // pair p = (i, i + 1 + j) after the walk over the rows of the triangle
    while (j >= m - 1 - i) {
      j -= m - 1 - i;
      ++i;
    }
    j += i + 1;
#pragma unroll 1
    for (int s0 = 0; s0 < S; s0 += SC) {
      if (type == RK_FIBINET_INTERACTION) dots(p, i, d, s0, pe, pv);
#pragma unroll
      for (int k = 0; k < SC; ++k) {
        const int s = s0 + k;
        if (type != RK_FIBINET_INTERACTION) {
          pe[k] = us[s * ldu + i * D + d];
          pv[k] = uv[s * ldu + i * D + d];
        }
        const float ej = es[s * lde + j * D + d];
        if (s < srows) {
          out[s * ldo + it] = pe[k] * ej;
          out[s * ldo + P * D + it] = pv[k] * (at[s * kA + j] * ej);
        }
      }
    }
  }
}

struct FibiArgs {
  FibiFields f;
  FibiWeights w;
  int64_t batch;
  float* c;
  int64_t ldc;
  float* linear;
  float* attn;
  int64_t ld_attn;
  uint32_t* flags;
};
static_assert(sizeof(FibiArgs) <= 4096, "kernel arguments beyond 4 KiB");

template <int S>
__global__ __launch_bounds__(kFibiThreads) void fibinet_interaction_kernel(FibiArgs a) {
  extern __shared__ __attribute__((aligned(16))) float fibi_smem[];
  const int tid = threadIdx.x;
  const int m = a.w.m, D = a.w.D, G = D >> 2;
  const int lde = m * D, ldu = (m - 1) * D;
  float* es = fibi_smem;
  float* us = es + S * lde;
  float* uv = us + (a.w.type == RK_FIBINET_INTERACTION ? 0 : S * ldu);
  float* zs = uv + (a.w.type == RK_FIBINET_INTERACTION ? 0 : S * ldu);
  float* hs = zs + S * kFibiMaxReduced;
  float* at = hs + S * kFibiMaxReduced;
  const int64_t b0 = (int64_t)blockIdx.x * S;
  const int srows = (int)min<int64_t>(S, a.batch - b0);
  for (int it = tid; it < S * m * G; it += kFibiThreads) {
    const int s = it / (m * G), rem = it - s * (m * G);
    const int i = rem / G, g = rem - i * G;
    *reinterpret_cast<f32x4*>(es + s * lde + i * D + 4 * g) = fibi_row4(a.f, i, b0 + s, a.batch, 4 * g, a.flags);
  }
  if (a.linear && tid < srows) a.linear[b0 + tid] = fibi_first_order(a.f, m, b0 + tid, a.flags);
  mlp_lds_barrier();
  fibi_interact<S, kFibiThreads>(a.w, es, us, uv, zs, hs, at, a.c + b0 * a.ldc, a.ldc, srows,
                                 a.attn ? a.attn + b0 * a.ld_attn : nullptr, a.ld_attn, tid);
}

struct FibiFwdArgs {
  FibiFields f;
  FibiWeights w;
  rk_mlp_layer L[RK_MLP_MAX_LAYERS];
  int nl;
  int64_t batch;
  int ld0, ld1;  // LDS row strides of the two activation buffers (floats)
  const float* head_w;
  const float* head_b;
  const float* final_w;  // [2]: linear, deep
  const float* final_b;
  float* linear;
  float* deep;
  float* logit;
  float* prob;
  uint32_t* flags;
};
static_assert(sizeof(FibiFwdArgs) <= 4096, "kernel arguments beyond 4 KiB");

__global__ __launch_bounds__(kMlpThreads) void fibinet_forward_kernel(FibiFwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  constexpr int S = kMlpRows;
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
  const int m = a.w.m, D = a.w.D, G = D >> 2;
  const int lde = m * D, ldu = (m - 1) * D;
  const int width = m * (m - 1) * D, K0p = pad64(width);
  const int64_t m0 = (int64_t)blockIdx.x * S;
  const int rows = (int)min<int64_t>(S, a.batch - m0);
  float* const buf0 = sm;
  float* const buf1 = buf0 + S * a.ld0;
  float* const es = buf1 + S * a.ld1;
  float* const us = es + S * lde;
  float* const uv = us + (a.w.type == RK_FIBINET_INTERACTION ? 0 : S * ldu);
  float* const zs = uv + (a.w.type == RK_FIBINET_INTERACTION ? 0 : S * ldu);
  float* const hs = zs + S * kFibiMaxReduced;
  float* const at = hs + S * kFibiMaxReduced;
  float* const lin = at + S * kFibiMaxReduced;

  // the gather: one float4 of a row per thread (16 m D / 4 <= 1024: the host checks), the first-order
  // sums by the last wave; loaded ahead of layer 0's weight ring, stored behind it (mlp_rows' stage)
  const bool gathers = tid < S * m * G;
  const int gs = tid / (m * G), grem = tid - gs * (m * G);
  const int gi = grem / G, gg = grem - gi * G;
  f32x4 gv = {0.f, 0.f, 0.f, 0.f};
  float lv = 0.f;
  auto issue = [&]() {
    if (gathers) gv = fibi_row4(a.f, gi, m0 + gs, a.batch, 4 * gg, a.flags);
    if (wave == kMlpWaves - 1 && lane < rows) lv = fibi_first_order(a.f, m, m0 + lane, a.flags);
  };
  auto finish = [&]() {
    if (gathers) *reinterpret_cast<f32x4*>(es + gs * lde + gi * D + 4 * gg) = gv;
    if (wave == kMlpWaves - 1 && lane < S) {
      lin[lane] = lv;
      if (lane < rows && a.linear) a.linear[m0 + lane] = lv;
    }
    const int padc = K0p - width;  // the MLP input row's zero K pad
    for (int it = tid; it < S * padc; it += kMlpThreads) buf0[(it / padc) * a.ld0 + width + it % padc] = 0.f;
    mlp_lds_barrier();
    // every row of the tile (a row past the batch staged zeros: its c is zero)
    fibi_interact<S, kMlpThreads>(a.w, es, us, uv, zs, hs, at, buf0, a.ld0, S, nullptr, 0, tid);
  };
  const rk_epilogue none = {};
  mlp_rows<1, false>(a.L, a.nl, width, buf0, a.ld0, buf1, a.ld1, m0, rows, none, nullptr, 0, tid,
                     two_phase(issue, finish));

  // the head, one wave per row: deep_output_layer, then final_layer over [linear, deep]
  const float* fin = (a.nl & 1) ? buf1 : buf0;
  const int ldf = (a.nl & 1) ? a.ld1 : a.ld0;
  const int Kh = a.L[a.nl - 1].n;
  if (wave < rows) {
    float p = 0.f;
    for (int n = lane; n < Kh; n += 64) p = __builtin_fmaf(fin[wave * ldf + n], a.head_w[n], p);
    p = wave_sum(p);
    if (lane == 0) {
      const int64_t b = m0 + wave;
      const float deep = p + a.head_b[0];
      const float logit = __builtin_fmaf(deep, a.final_w[1], __builtin_fmaf(lin[wave], a.final_w[0], a.final_b[0]));
      if (a.deep) a.deep[b] = deep;
      if (a.logit) a.logit[b] = logit;
      if (a.prob) a.prob[b] = 1.0f / (1.0f + expf(-logit));
    }
  }
}

// Both entry points' front: the envelope, the segments and the weights.
int fibi_front(const char* name, const rk_segment* second_order, const rk_segment* first_order, int32_t num_fields,
               int32_t dim, int64_t batch, const float* senet_w1, const float* senet_w2, int32_t reduced,
               const float* bilinear_e, const float* bilinear_v, int32_t bilinear_type, bool want_first, FibiFields& t,
               FibiWeights& w) {
  if (!second_order || !senet_w1 || !senet_w2 || !bilinear_e || !bilinear_v)
    return fail(RK_ERR_INVALID, "%s: null segments or weights", name);
  if (batch < 0) return fail(RK_ERR_INVALID, "%s: negative batch", name);
  if (want_first && !first_order) return fail(RK_ERR_INVALID, "%s: the first-order sum needs first_order (null)", name);
  if (num_fields < 2 || num_fields > kFibiMaxFields)
    return fail(RK_ERR_UNSUPPORTED, "%s: %d fields outside [2, %d]", name, num_fields, kFibiMaxFields);
  if (dim < 4 || dim > kFibiMaxDim || dim % 4)
    return fail(RK_ERR_UNSUPPORTED, "%s: dim %d not a multiple of 4 in [4, %d]", name, dim, kFibiMaxDim);
  if (reduced < 1) return fail(RK_ERR_INVALID, "%s: reduced SENET width %d", name, reduced);
  if (reduced > kFibiMaxReduced)
    return fail(RK_ERR_UNSUPPORTED, "%s: reduced SENET width %d (max %d)", name, reduced, kFibiMaxReduced);
  if (bilinear_type != RK_FIBINET_ALL && bilinear_type != RK_FIBINET_EACH && bilinear_type != RK_FIBINET_INTERACTION)
    return fail(RK_ERR_INVALID, "%s: bilinear type %d", name, bilinear_type);
  if (!aligned16(bilinear_e) || !aligned16(bilinear_v))
    return fail(RK_ERR_INVALID, "%s: bilinear weights must be 16-B aligned", name);
  int dense = 0;
  for (int i = 0; i < num_fields; ++i) {
    const rk_segment& s = second_order[i];
    if (!s.src || s.dim != dim || s.src_ld % 4 || !aligned16(s.src) || (s.idx && s.rows <= 0))
      return fail(RK_ERR_INVALID, "%s: field %d layout (dim %d, 16-B aligned rows)", name, i, dim);
    dense += s.idx == nullptr;
    t.src2[i] = s.src;
    t.idx2[i] = s.idx;
    t.ld2[i] = s.src_ld;
    t.rows2[i] = s.rows;
    t.istride2[i] = s.idx_stride;
    t.src1[i] = nullptr;
    t.idx1[i] = nullptr;
    t.ld1[i] = t.rows1[i] = t.istride1[i] = 0;
    if (want_first) {
      const rk_segment& f = first_order[i];
      if (!f.src || f.dim != 1 || (f.idx && f.rows <= 0) || (f.idx == nullptr) != (s.idx == nullptr))
        return fail(RK_ERR_INVALID, "%s: first-order field %d", name, i);
      t.src1[i] = f.src;
      t.idx1[i] = f.idx;
      t.ld1[i] = f.src_ld;
      t.rows1[i] = f.rows;
      t.istride1[i] = f.idx_stride;
    }
  }
  if (dense != 0 && dense != num_fields)
    return fail(RK_ERR_UNSUPPORTED, "%s: segments must be all tables or all dense", name);
  w.w1 = senet_w1;
  w.w2 = senet_w2;
  w.be = bilinear_e;
  w.bv = bilinear_v;
  w.m = num_fields;
  w.D = dim;
  w.r = reduced;
  w.type = bilinear_type;
  return RK_OK;
}

}  // namespace
}  // namespace rk

using namespace rk;

RK_API int rk_fibinet_interaction(const rk_segment* second_order, const rk_segment* first_order, int32_t num_fields,
                                  int32_t dim, int64_t batch, const float* senet_w1, const float* senet_w2,
                                  int32_t reduced, const float* bilinear_e, const float* bilinear_v,
                                  int32_t bilinear_type, float* c, int64_t ldc, float* linear, float* attention,
                                  int64_t ld_attention, void* stream) {
  const char* name = "rk_fibinet_interaction";
  FibiArgs a = {};
  if (!c) return fail(RK_ERR_INVALID, "%s: null output", name);
  if (int rc = fibi_front(name, second_order, first_order, num_fields, dim, batch, senet_w1, senet_w2, reduced,
                          bilinear_e, bilinear_v, bilinear_type, linear != nullptr, a.f, a.w))
    return rc;
  const int64_t width = (int64_t)num_fields * (num_fields - 1) * dim;
  if (ldc < width || (attention && ld_attention < num_fields))
    return fail(RK_ERR_INVALID, "%s: ldc %lld < %lld, or ld_attention %lld < %d", name, (long long)ldc, (long long)width,
                (long long)ld_attention, num_fields);
  a.batch = batch;
  a.c = c;
  a.ldc = ldc;
  a.linear = linear;
  a.attn = attention;
  a.ld_attn = ld_attention;
  a.flags = device_flags();
  if (!a.flags) return fail(RK_ERR_RUNTIME, "%s: device not initialised (rk_init)", name);
  if (batch == 0) return RK_OK;
  // 16 samples per workgroup while their rows and products fit the LDS, else 4 (32 x 64: 97 KiB)
  const bool s16 = batch > 4 && fibi_tile_floats(16, num_fields, dim, bilinear_type) * 4 <= kFibiLdsBytes;
  const int S = s16 ? 16 : 4;
  const int lds = fibi_tile_floats(S, num_fields, dim, bilinear_type) * 4;
  if (lds > kFibiLdsBytes) return fail(RK_ERR_UNSUPPORTED, "%s: LDS budget", name);
  const int64_t blocks = (batch + S - 1) / S;
  if (blocks > INT32_MAX) return fail(RK_ERR_UNSUPPORTED, "%s: batch too large", name);
  if (s16) {
    raise_lds_limit((const void*)fibinet_interaction_kernel<16>, kFibiLdsBytes);
    fibinet_interaction_kernel<16><<<(unsigned)blocks, kFibiThreads, lds, (hipStream_t)stream>>>(a);
  } else {
    raise_lds_limit((const void*)fibinet_interaction_kernel<4>, kFibiLdsBytes);
    fibinet_interaction_kernel<4><<<(unsigned)blocks, kFibiThreads, lds, (hipStream_t)stream>>>(a);
  }
  return check_launch(name);
}

RK_API int rk_fibinet_forward(const rk_segment* second_order, const rk_segment* first_order, int32_t num_fields,
                              int32_t dim, int64_t batch, const float* senet_w1, const float* senet_w2,
                              int32_t reduced, const float* bilinear_e, const float* bilinear_v,
                              int32_t bilinear_type, const rk_mlp_layer* layers, int32_t nlayers, const float* head_w,
                              const float* head_b, const float* final_w, const float* final_b, float* linear,
                              float* deep_logit, float* total_logit, float* prob, void* stream) {
  const char* name = "rk_fibinet_forward";
  FibiFwdArgs a = {};
  if (!layers || !head_w || !head_b || !final_w || !final_b)
    return fail(RK_ERR_INVALID, "%s: null layers or head", name);
  if (!(linear || deep_logit || total_logit || prob)) return fail(RK_ERR_INVALID, "%s: no output", name);
  if (int rc = fibi_front(name, second_order, first_order, num_fields, dim, batch, senet_w1, senet_w2, reduced,
                          bilinear_e, bilinear_v, bilinear_type, true, a.f, a.w))
    return rc;
  if (nlayers < 1) return fail(RK_ERR_UNSUPPORTED, "%s: %d hidden layers (1..%d)", name, nlayers, RK_MLP_MAX_LAYERS);
  const int64_t width = (int64_t)num_fields * (num_fields - 1) * dim;
  if (width > 1024) return fail(RK_ERR_UNSUPPORTED, "%s: interaction width %lld > 1024", name, (long long)width);
  if (kMlpRows * num_fields * (dim / 4) > kMlpThreads)
    return fail(RK_ERR_UNSUPPORTED, "%s: %d x %d rows beyond one float4 per thread", name, num_fields, dim);
  const rk_epilogue none = {};
  int need0 = 0, need1 = 0;
  if (int e = mlp_validate(layers, nlayers, (int)width, none, &need0, &need1, name)) return e;
  for (int l = 0; l < nlayers; ++l) {
    if (layers[l].store || layers[l].residual)
      return fail(RK_ERR_UNSUPPORTED, "%s: eval only, no residual (layer %d)", name, l);
    a.L[l] = layers[l];
  }
  a.nl = nlayers;
  a.ld0 = need0 + kMlpLdPad;
  a.ld1 = need1 + kMlpLdPad;
  const size_t shm = ((size_t)kMlpRows * (a.ld0 + a.ld1) + fibi_tile_floats(kMlpRows, num_fields, dim, bilinear_type) +
                      kMlpRows) * sizeof(float);
  if (shm > (size_t)kFibiLdsBytes) return fail(RK_ERR_UNSUPPORTED, "%s: widths need %zu B of LDS", name, shm);
  a.batch = batch;
  a.head_w = head_w;
  a.head_b = head_b;
  a.final_w = final_w;
  a.final_b = final_b;
  a.linear = linear;
  a.deep = deep_logit;
  a.logit = total_logit;
  a.prob = prob;
  a.flags = device_flags();
  if (!a.flags) return fail(RK_ERR_RUNTIME, "%s: device not initialised (rk_init)", name);
  if (batch == 0) return RK_OK;
  const int64_t blocks = (batch + kMlpRows - 1) / kMlpRows;
  if (blocks > INT32_MAX) return fail(RK_ERR_UNSUPPORTED, "%s: batch too large", name);
  raise_lds_limit((const void*)fibinet_forward_kernel, kFibiLdsBytes);
  fibinet_forward_kernel<<<(unsigned)blocks, kMlpThreads, shm, (hipStream_t)stream>>>(a);
  return check_launch(name);
}
