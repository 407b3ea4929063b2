// Backward of xDeepFM's Compressed Interaction Network (cin.hip): rk_cin_backward (the gradient of the
// rows x0 and every layer's dy), rk_cin_wgrad (dW_k, dbias_k) and rk_cin_pack_weight_t.
//
// Saved by rk_cin_forward_train: maps[b][off_k + n][d] = x^k[n, (b, d)], sample stride hsum * D
// (hsum = sum H_k, off_k = H_1 + .. + H_{k-1}); dy has the same layout.  x0 is [B, m D] rows.
//
// Data backward.  A workgroup owns a tile of NC columns c = s D + d as in the forward; x0, dx0 and two
// buffers [Hmax16][NC] (dy^k in one, dy^{k-1} being built in the other) stay in LDS.  With
//   T_i[h, c] = sum_n W_k[n, h m + i] dy^k[n, c]
// the two products of the layer are g^{k-1}[h, c] = sum_i x0[i, c] T_i[h, c] and
// dx0[i, c] += sum_h x^{k-1}[h, c] T_i[h, c].  rk_cin_pack_weight_t lays W_k^T out field-major (rows
// (i, h), H_{k-1} padded to 16 per field) in the A-operand order of v_mfma_f32_16x16x4_f32, so one
// output tile holds T_i for 16 values of h at one field i.  A wave owns one 16-column tile of the
// workgroup for every layer: per 16-row tile of h it loops the fields (four accumulators at a time,
// one LDS read of dy^k per four MFMAs), adds x0[i, c] * T into a register accumulator of g^{k-1}, and
// reduces x^{k-1}[h, c] * T over its rows (in lane, then across the four lane groups) into dx0[i, c]
// in LDS, row tiles in order.  Only that wave touches those columns, so there is no barrier between
// layers, no atomic and one summation order.  z, dz and T never leave registers.
//
// Weight gradient.  dW_k[n, h m + i] = sum_c dy^k[n, c] x^{k-1}[h, c] x0[i, c]: a workgroup owns all
// rows n and 128 columns j of one layer for a slab of the B D reduction, stages 64 reduction columns
// at a time (dy^k, the rows of x^{k-1} its j range needs, x0), forms the z operand as a product of
// two LDS reads, and writes its partial tile to a workspace; rk_cin_wgrad's second kernel sums the at
// most kCwMaxSlabs partials in slab order.  dbias_k comes from the staged dy^k (wave sums, fixed order).
#include "common.h"

namespace rk {
namespace {

constexpr int kCbMaxFields = 32;
constexpr int kCbMaxLayers = 4;
constexpr int kCbMaxMaps = 256;
constexpr int kCbThreads = 512;
constexpr int kCbWaves = kCbThreads / kWave;
constexpr int kCbLdsBytes = 160 * 1024;

constexpr int kCwNC = 64;            // reduction columns per staged step
constexpr int kCwNQ = kCwNC / 4;
constexpr int kCwPitch = kCwNC + 4;  // the 16 rows x 4 columns of an A read fall on 64 distinct banks
constexpr int kCwJB = 128;           // output columns j per workgroup: 16 per wave
constexpr int kCwMaxSlabs = 32;      // partial tiles per output element (bounds the workspace)
constexpr int kCwXRows = kCwJB / 2 + 2;  // rows of x^{k-1} a j block can touch (m >= 2)

struct CbLayers {
  const float* wt[kCbMaxLayers];  // rk_cin_pack_weight_t images
  int32_t h[kCbMaxLayers];
};

struct CwLayers {
  int32_t h[kCbMaxLayers];
  int64_t woff[kCbMaxLayers];  // offset of dW_k in a slab's partial block
  float* dw[kCbMaxLayers];
  float* dbias[kCbMaxLayers];
};

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// One wave, one 16-column tile, the 16 rows h of tile ht, fields i0 .. i0 + NB - 1: T_i over the whole
// K = pad16(H_k) loop, then the two products.
template <int NB>
__device__ __forceinline__ void cin_bwd_unit(const float* __restrict__ Wt, int KS4, int MTp, int ht, int i0,
                                             const float* cur, const float* x0, float* dx0, int ld, int c, int lane,
                                             const float (&xprev)[4], float (&gacc)[4]) {
  f32x4 acc[NB];
#pragma unroll
  for (int t = 0; t < NB; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const f32x4* wp = reinterpret_cast<const f32x4*>(Wt) + ((int64_t)i0 * MTp + ht) * KS4 * kWave + lane;
  const int64_t tstride = (int64_t)MTp * KS4 * kWave;
  const float* bp = cur + (lane >> 4) * ld + c;
  for (int ks4 = 0; ks4 < KS4; ++ks4) {
    f32x4 a[NB];
#pragma unroll
    for (int t = 0; t < NB; ++t) a[t] = wp[t * tstride + (int64_t)ks4 * kWave];
    float bv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) bv[e] = bp[(ks4 * 16 + e * 4) * ld];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
#pragma unroll
      for (int t = 0; t < NB; ++t) acc[t] = mfma16(a[t][e], bv[e], acc[t]);
    }
  }
#pragma unroll
  for (int t = 0; t < NB; ++t) {
    const int i = i0 + t;
    const float x0v = x0[i * ld + c];
    float p = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      gacc[r] = fmaf(x0v, acc[t][r], gacc[r]);
      p = fmaf(xprev[r], acc[t][r], p);
    }
    p += __shfl_xor(p, 16, kWave);
    p += __shfl_xor(p, 32, kWave);
    if (lane < 16) dx0[i * ld + c] += p;
  }
}

template <int NC>
__global__ __launch_bounds__(kCbThreads) void cin_backward_kernel(
    const CbLayers L, const float* __restrict__ x0g, int64_t ld_x0, int m, int D, int nlayers, int act, int ld,
    int hp_max, int hsum, int64_t batch, const float* __restrict__ maps, const float* __restrict__ dpooled,
    int64_t ld_dp, const float* __restrict__ dlogit, const float* __restrict__ out_w,
    const float* __restrict__ dx0_add, int64_t ld_add, float* __restrict__ dx0g, int64_t ld_dx0,
    float* __restrict__ dy) {
  extern __shared__ __attribute__((aligned(16))) float cb_smem[];
  constexpr int NQ = NC / 4;
  constexpr int NT = NC / 16;
  float* x0 = cb_smem;               // [m][ld]
  float* dx0 = x0 + m * ld;          // [m][ld]
  float* bufA = dx0 + m * ld;        // [hp_max][ld]
  float* bufB = bufA + hp_max * ld;  // [hp_max][ld]
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
  const int G = D >> 2;
  const int S = NC / D;
  const int64_t b0 = (int64_t)blockIdx.x * S;
  const bool relu = act == RK_ACT_RELU;

  // the upstream gradient of x^k[n, (b, d)] through the pooling: dpooled and / or dlogit * out_w
  auto dpool = [&](int64_t b, int col) {
    float v = dpooled ? dpooled[b * ld_dp + col] : 0.f;
    if (dlogit) v = fmaf(dlogit[b], out_w[col], v);
    return v;
  };

  for (int it = tid; it < m * NQ; it += kCbThreads) {
    const int c4 = it % NQ, i = it / NQ;
    const int s = c4 / G, d0 = (c4 - s * G) * 4;
    const int64_t b = b0 + s;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (b < batch) v = *reinterpret_cast<const f32x4*>(x0g + b * ld_x0 + i * D + d0);
    *reinterpret_cast<f32x4*>(x0 + i * ld + c4 * 4) = v;
    *reinterpret_cast<f32x4*>(dx0 + i * ld + c4 * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  {  // dy of the last layer (rows up to pad16(H) zero)
    const int H = L.h[nlayers - 1], Hp = (H + 15) & ~15, off = hsum - H;
    for (int id = tid; id < Hp * NQ; id += kCbThreads) {
      const int c4 = id % NQ, n = id / NQ;
      const int s = c4 / G, d0 = (c4 - s * G) * 4;
      const int64_t b = b0 + s;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (n < H && b < batch) {
        const float dp = dpool(b, off + n);
        v = f32x4{dp, dp, dp, dp};
        const int64_t at = (b * hsum + off + n) * D + d0;
        if (relu) {
          const f32x4 xm = *reinterpret_cast<const f32x4*>(maps + at);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = xm[e] > 0.f ? dp : 0.f;
        }
        *reinterpret_cast<f32x4*>(dy + at) = v;
      }
      *reinterpret_cast<f32x4*>(bufA + n * ld + c4 * 4) = v;
    }
  }
  __syncthreads();

  if (wave < NT) {  // this wave's 16 columns, every layer: no other wave reads or writes them
    const int c = wave * 16 + (lane & 15);
    const int s = c / D, d = c - s * D;
    const int64_t b = b0 + s;
    const bool valid = b < batch;
    float* cur = bufA;
    float* other = bufB;
    int off = hsum;
    for (int k = nlayers - 1; k >= 0; --k) {
      const int H = L.h[k];
      off -= H;  // off_k
      const int hprev = k > 0 ? L.h[k - 1] : m;
      const int off_prev = off - hprev;  // k > 0 only
      const int MTp = (hprev + 15) >> 4, KS4 = (H + 15) >> 4;
      for (int ht = 0; ht < MTp; ++ht) {
        const int hbase = ht * 16 + 4 * (lane >> 4);
        float xprev[4], gacc[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int h = hbase + r;
          gacc[r] = 0.f;
          if (k > 0)
            xprev[r] = (valid && h < hprev) ? maps[(b * hsum + off_prev + h) * D + d] : 0.f;
          else
            xprev[r] = h < m ? x0[h * ld + c] : 0.f;
        }
        for (int i0 = 0; i0 < m; i0 += 4) {
          switch (min(4, m - i0)) {
            case 1: cin_bwd_unit<1>(L.wt[k], KS4, MTp, ht, i0, cur, x0, dx0, ld, c, lane, xprev, gacc); break;
            case 2: cin_bwd_unit<2>(L.wt[k], KS4, MTp, ht, i0, cur, x0, dx0, ld, c, lane, xprev, gacc); break;
            case 3: cin_bwd_unit<3>(L.wt[k], KS4, MTp, ht, i0, cur, x0, dx0, ld, c, lane, xprev, gacc); break;
            default: cin_bwd_unit<4>(L.wt[k], KS4, MTp, ht, i0, cur, x0, dx0, ld, c, lane, xprev, gacc); break;
          }
        }
        // the wave's LDS operations complete in program order; keep the compiler to it as well
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (k > 0) {  // dy^{k-1} = (pooling gradient + g^{k-1}) * act'(x^{k-1}); rows past H_{k-1} zero
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int h = hbase + r;
            float v = 0.f;
            if (valid && h < hprev) {
              v = dpool(b, off_prev + h) + gacc[r];
              if (relu && !(xprev[r] > 0.f)) v = 0.f;
              dy[(b * hsum + off_prev + h) * D + d] = v;
            }
            other[h * ld + c] = v;
          }
        } else {  // g^0 is a gradient of x0 as well
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int h = hbase + r;
            if (h < m) dx0[h * ld + c] += gacc[r];
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
      }
      float* t = cur;
      cur = other;
      other = t;
    }
  }
  __syncthreads();
  for (int it = tid; it < m * NQ; it += kCbThreads) {
    const int c4 = it % NQ, i = it / NQ;
    const int s = c4 / G, d0 = (c4 - s * G) * 4;
    const int64_t b = b0 + s;
    if (b >= batch) continue;
    f32x4 v = *reinterpret_cast<const f32x4*>(dx0 + i * ld + c4 * 4);
    if (dx0_add) v += *reinterpret_cast<const f32x4*>(dx0_add + b * ld_add + i * D + d0);
    *reinterpret_cast<f32x4*>(dx0g + b * ld_dx0 + i * D + d0) = v;
  }
}

// out[((rt * KS4 + ks4) * 64 + lane) * 4 + e] = W[n][h m + i] with row rt * 16 + lane % 16 = i * Hp + h
// (Hp = pad16(hprev)) and n = ks4 * 16 + 4 e + lane / 16; zero past hprev / n.
__global__ __launch_bounds__(256) void cin_pack_weight_t_kernel(const float* __restrict__ w, int64_t ldw, int n,
                                                                int hprev, int m, int Hp, int KS4, int64_t total,
                                                                float* __restrict__ out) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= total) return;
  const int e = (int)(o & 3), lane = (int)((o >> 2) & 63);
  const int64_t blk = o >> 8;  // rt * KS4 + ks4
  const int ks4 = (int)(blk % KS4), rt = (int)(blk / KS4);
  const int row = rt * 16 + (lane & 15), col = ks4 * 16 + e * 4 + (lane >> 4);
  const int i = row / Hp, h = row - i * Hp;
  out[o] = (i < m && h < hprev && col < n) ? w[col * ldw + h * m + i] : 0.f;
}

// grid (slabs, j blocks, layers)
__global__ __launch_bounds__(kCbThreads) void cin_wgrad_kernel(const CwLayers L, const float* __restrict__ x0g,
                                                               int64_t ld_x0, int m, int D, int hsum, int64_t batch,
                                                               int64_t tiles, int64_t tps,
                                                               const float* __restrict__ maps,
                                                               const float* __restrict__ dy, float* __restrict__ ws,
                                                               int64_t slab_floats, int64_t wtot) {
  __shared__ __attribute__((aligned(16))) float dyS[kCbMaxMaps * kCwPitch];
  __shared__ __attribute__((aligned(16))) float xS[kCwXRows * kCwPitch];
  __shared__ __attribute__((aligned(16))) float x0S[kCbMaxFields * kCwPitch];
  __shared__ float bsumS[kCbMaxMaps];
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
  const int k = blockIdx.z;
  const int H = L.h[k], hprev = k > 0 ? L.h[k - 1] : m;
  const int Kk = hprev * m;
  const int j0 = blockIdx.y * kCwJB;
  if (j0 >= Kk) return;
  int off = 0;
  for (int q = 0; q < k; ++q) off += L.h[q];
  const int off_prev = off - hprev;  // k > 0 only
  const int MT = (H + 15) >> 4;
  const int G = D >> 2, S = kCwNC / D;
  const int h_lo = j0 / m, h_hi = min(hprev - 1, (j0 + kCwJB - 1) / m);
  const int xrows = h_hi - h_lo + 1;
  const int j = j0 + 16 * wave + (lane & 15);
  const bool jok = j < Kk;
  const int hj = jok ? j / m : h_lo, ij = jok ? j - hj * m : 0;
  const bool bias = blockIdx.y == 0;
  if (tid < kCbMaxMaps) bsumS[tid] = 0.f;
  f32x4 acc[kCbMaxMaps / 16];
#pragma unroll
  for (int t = 0; t < kCbMaxMaps / 16; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int64_t t0 = (int64_t)blockIdx.x * tps, t1 = min<int64_t>(tiles, t0 + tps);
  for (int64_t tile = t0; tile < t1; ++tile) {
    const int64_t b0 = tile * S;
    for (int id = tid; id < MT * 16 * kCwNQ; id += kCbThreads) {
      const int c4 = id % kCwNQ, n = id / kCwNQ;
      const int s = c4 / G, d0 = (c4 - s * G) * 4;
      const int64_t b = b0 + s;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (n < H && b < batch) v = *reinterpret_cast<const f32x4*>(dy + (b * hsum + off + n) * D + d0);
      *reinterpret_cast<f32x4*>(dyS + n * kCwPitch + c4 * 4) = v;
    }
    for (int id = tid; id < xrows * kCwNQ; id += kCbThreads) {
      const int c4 = id % kCwNQ, hh = h_lo + id / kCwNQ;
      const int s = c4 / G, d0 = (c4 - s * G) * 4;
      const int64_t b = b0 + s;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (b < batch)
        v = k > 0 ? *reinterpret_cast<const f32x4*>(maps + (b * hsum + off_prev + hh) * D + d0)
                  : *reinterpret_cast<const f32x4*>(x0g + b * ld_x0 + hh * D + d0);
      *reinterpret_cast<f32x4*>(xS + (hh - h_lo) * kCwPitch + c4 * 4) = v;
    }
    for (int id = tid; id < m * kCwNQ; id += kCbThreads) {
      const int c4 = id % kCwNQ, i = id / kCwNQ;
      const int s = c4 / G, d0 = (c4 - s * G) * 4;
      const int64_t b = b0 + s;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (b < batch) v = *reinterpret_cast<const f32x4*>(x0g + b * ld_x0 + i * D + d0);
      *reinterpret_cast<f32x4*>(x0S + i * kCwPitch + c4 * 4) = v;
    }
    __syncthreads();
    if (bias) {  // row n belongs to wave n % 8 for the whole slab: one order
      for (int n = wave; n < H; n += kCbWaves) {
        const float sum = wave_sum(dyS[n * kCwPitch + lane]);
        if (lane == 0) bsumS[n] += sum;
      }
    }
    for (int s4 = 0; s4 < kCwNC / 4; ++s4) {
      const int cc = 4 * s4 + (lane >> 4);
      const float bv = jok ? xS[(hj - h_lo) * kCwPitch + cc] * x0S[ij * kCwPitch + cc] : 0.f;
#pragma unroll
      for (int t = 0; t < kCbMaxMaps / 16; ++t) {
        if (t < MT) acc[t] = mfma16(dyS[(16 * t + (lane & 15)) * kCwPitch + cc], bv, acc[t]);
      }
    }
    __syncthreads();
  }
  float* out = ws + (int64_t)blockIdx.x * slab_floats;
#pragma unroll
  for (int t = 0; t < kCbMaxMaps / 16; ++t) {
    if (t < MT) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = 16 * t + 4 * (lane >> 4) + r;
        if (n < H && jok) out[L.woff[k] + (int64_t)n * Kk + j] = acc[t][r];
      }
    }
  }
  if (bias && tid < H) out[wtot + off + tid] = bsumS[tid];
}

// dW_k, dbias_k = the slabs' partials added in slab order
__global__ __launch_bounds__(256) void cin_wgrad_reduce_kernel(const CwLayers L, int nlayers, int m,
                                                               const float* __restrict__ ws, int64_t slab_floats,
                                                               int64_t wtot, int slabs) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= slab_floats) return;
  float s = 0.f;
  for (int q = 0; q < slabs; ++q) s += ws[(int64_t)q * slab_floats + e];
  if (e < wtot) {
    int k = nlayers - 1;
    while (k > 0 && e < L.woff[k]) --k;
    L.dw[k][e - L.woff[k]] = s;
  } else {
    int64_t n = e - wtot;
    int k = 0;
    while (n >= L.h[k]) n -= L.h[k++];
    if (L.dbias[k]) L.dbias[k][n] = s;
  }
}

// The envelope shared by the three entries (rk_cin_forward's); fills hmax / hsum.
int cin_bwd_envelope(const char* who, int32_t num_fields, int32_t dim, const int32_t* layer_sizes,
                     int32_t num_layers, int64_t batch, int* hmax, int* hsum) {
  if (!layer_sizes || num_fields <= 0 || num_layers <= 0 || dim <= 0)
    return fail(RK_ERR_INVALID, "%s: null layer sizes or a non-positive count", who);
  if (num_fields < 2 || num_fields > kCbMaxFields)
    return fail(RK_ERR_UNSUPPORTED, "%s: %d fields outside [2, %d]", who, num_fields, kCbMaxFields);
  if (dim != 4 && dim != 8 && dim != 16 && dim != 32 && dim != 64)
    return fail(RK_ERR_UNSUPPORTED, "%s: dim %d not in {4, 8, 16, 32, 64}", who, dim);
  if (num_layers > kCbMaxLayers) return fail(RK_ERR_UNSUPPORTED, "%s: %d layers (max %d)", who, num_layers, kCbMaxLayers);
  *hmax = *hsum = 0;
  for (int k = 0; k < num_layers; ++k) {
    const int h = layer_sizes[k];
    if (h <= 0) return fail(RK_ERR_INVALID, "%s: layer %d has %d maps", who, k, h);
    if (h > kCbMaxMaps) return fail(RK_ERR_UNSUPPORTED, "%s: layer %d has %d maps (max %d)", who, k, h, kCbMaxMaps);
    *hmax = std::max(*hmax, h);
    *hsum += h;
  }
  if (batch < 0) return fail(RK_ERR_INVALID, "%s: negative batch", who);
  return RK_OK;
}

int64_t cin_wgrad_slab_floats(int32_t m, const int32_t* sizes, int32_t nl, int64_t* wtot) {
  int64_t w = 0, hs = 0;
  int hprev = m;
  for (int k = 0; k < nl; ++k) {
    w += (int64_t)sizes[k] * hprev * m;
    hs += sizes[k];
    hprev = sizes[k];
  }
  if (wtot) *wtot = w;
  return w + hs;
}

}  // namespace
}  // namespace rk

using namespace rk;

RK_API int rk_cin_pack_weight_t(const float* w, int64_t ldw, int32_t n, int32_t hprev, int32_t num_fields, float* out,
                                void* stream) {
  if (!w || !out || n <= 0 || hprev <= 0 || num_fields <= 0 || ldw < (int64_t)hprev * num_fields || !aligned16(out))
    return fail(RK_ERR_INVALID, "rk_cin_pack_weight_t: bad arguments (n=%d hprev=%d fields=%d ldw=%lld)", n, hprev,
                num_fields, (long long)ldw);
  const int Hp = (hprev + 15) / 16 * 16, KS4 = (n + 15) / 16;
  const int64_t total = (int64_t)num_fields * Hp * KS4 * 16;
  const int64_t blocks = (total + 255) / 256;
  if (blocks > INT32_MAX) return fail(RK_ERR_UNSUPPORTED, "rk_cin_pack_weight_t: weight too large");
  cin_pack_weight_t_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(w, ldw, n, hprev, num_fields, Hp, KS4,
                                                                             total, out);
  return check_launch("rk_cin_pack_weight_t");
}

RK_API int rk_cin_backward(const float* x0, int64_t ld_x0, int32_t num_fields, int32_t dim, int64_t batch,
                           const float* const* weights_t, const int32_t* layer_sizes, int32_t num_layers,
                           int32_t activation, const float* maps, const float* dpooled, int64_t ld_dpooled,
                           const float* dlogit, const float* out_w, const float* dx0_add, int64_t ld_add, float* dx0,
                           int64_t ld_dx0, float* dy, void* stream) {
  if (!weights_t) return fail(RK_ERR_INVALID, "rk_cin_backward: null weight images");
  int hmax, hsum;
  if (int rc = cin_bwd_envelope("rk_cin_backward", num_fields, dim, layer_sizes, num_layers, batch, &hmax, &hsum)) return rc;
  if (activation != RK_ACT_NONE && activation != RK_ACT_RELU)
    return fail(RK_ERR_UNSUPPORTED, "rk_cin_backward: activation %d (identity or ReLU)", activation);
  CbLayers L;
  for (int k = 0; k < kCbMaxLayers; ++k) {
    L.wt[k] = nullptr;
    L.h[k] = 0;
  }
  for (int k = 0; k < num_layers; ++k) {
    if (!weights_t[k] || !aligned16(weights_t[k]))
      return fail(RK_ERR_INVALID, "rk_cin_backward: layer %d weight image", k);
    L.wt[k] = weights_t[k];
    L.h[k] = layer_sizes[k];
  }
  const int64_t width = (int64_t)num_fields * dim;
  if (!x0 || !maps || !dx0 || !dy || (!dpooled && !dlogit) || (dlogit && !out_w))
    return fail(RK_ERR_INVALID, "rk_cin_backward: null x0 / maps / dx0 / dy, or no upstream gradient");
  if (!aligned16(x0) || !aligned16(maps) || !aligned16(dx0) || !aligned16(dy) || !aligned16(dx0_add) || ld_x0 % 4 ||
      ld_dx0 % 4 || ld_x0 < width || ld_dx0 < width || (dx0_add && (ld_add % 4 || ld_add < width)))
    return fail(RK_ERR_INVALID, "rk_cin_backward: rows must be 16-B aligned with strides %% 4 == 0, >= %lld",
                (long long)width);
  if (dpooled && ld_dpooled < hsum)
    return fail(RK_ERR_INVALID, "rk_cin_backward: ld_dpooled %lld < %d", (long long)ld_dpooled, hsum);
  if (batch == 0) return RK_OK;
  const int hp = (hmax + 15) / 16 * 16;
  auto bytes = [&](int nc, int pad) { return (int64_t)(2 * hp + 2 * num_fields) * (nc + pad) * 4; };
  int nc = 128, pad = 16;
  if (batch * dim <= 64 || bytes(nc, pad) > kCbLdsBytes) nc = 64;
  if (bytes(nc, pad) > kCbLdsBytes) pad = 0;
  if (bytes(nc, pad) > kCbLdsBytes) return fail(RK_ERR_UNSUPPORTED, "rk_cin_backward: LDS budget");
  const int S = nc / dim;
  const int64_t blocks = (batch + S - 1) / S;
  if (blocks > INT32_MAX) return fail(RK_ERR_UNSUPPORTED, "rk_cin_backward: batch too large");
  const int lds = (int)bytes(nc, pad);
  hipStream_t st = (hipStream_t)stream;
  if (nc == 128) {
    raise_lds_limit((const void*)cin_backward_kernel<128>, lds);
    cin_backward_kernel<128><<<(unsigned)blocks, kCbThreads, lds, st>>>(
        L, x0, ld_x0, num_fields, dim, num_layers, activation, nc + pad, hp, hsum, batch, maps, dpooled, ld_dpooled,
        dlogit, out_w, dx0_add, ld_add, dx0, ld_dx0, dy);
  } else {
    raise_lds_limit((const void*)cin_backward_kernel<64>, lds);
    cin_backward_kernel<64><<<(unsigned)blocks, kCbThreads, lds, st>>>(
        L, x0, ld_x0, num_fields, dim, num_layers, activation, nc + pad, hp, hsum, batch, maps, dpooled, ld_dpooled,
        dlogit, out_w, dx0_add, ld_add, dx0, ld_dx0, dy);
  }
  return check_launch("rk_cin_backward");
}

RK_API int64_t rk_cin_wgrad_workspace_floats(int32_t num_fields, const int32_t* layer_sizes, int32_t num_layers) {
  if (!layer_sizes || num_fields <= 0 || num_layers <= 0 || num_layers > kCbMaxLayers) return 0;
  for (int k = 0; k < num_layers; ++k)
    if (layer_sizes[k] <= 0) return 0;
  return kCwMaxSlabs * cin_wgrad_slab_floats(num_fields, layer_sizes, num_layers, nullptr);
}

RK_API int rk_cin_wgrad(const float* x0, int64_t ld_x0, int32_t num_fields, int32_t dim, int64_t batch,
                        const int32_t* layer_sizes, int32_t num_layers, const float* maps, const float* dy,
                        float* const* dw, float* const* dbias, float* workspace, int64_t workspace_floats,
                        void* stream) {
  if (!dw) return fail(RK_ERR_INVALID, "rk_cin_wgrad: null gradient pointers");
  int hmax, hsum;
  if (int rc = cin_bwd_envelope("rk_cin_wgrad", num_fields, dim, layer_sizes, num_layers, batch, &hmax, &hsum)) return rc;
  CwLayers L;
  int64_t wtot = 0;
  const int64_t slab_floats = cin_wgrad_slab_floats(num_fields, layer_sizes, num_layers, &wtot);
  int hprev = num_fields, kmax = 0;
  int64_t woff = 0;
  for (int k = 0; k < kCbMaxLayers; ++k) {
    L.h[k] = 0;
    L.woff[k] = 0;
    L.dw[k] = L.dbias[k] = nullptr;
  }
  for (int k = 0; k < num_layers; ++k) {
    if (!dw[k]) return fail(RK_ERR_INVALID, "rk_cin_wgrad: layer %d has no gradient buffer", k);
    L.h[k] = layer_sizes[k];
    L.woff[k] = woff;
    L.dw[k] = dw[k];
    L.dbias[k] = dbias ? dbias[k] : nullptr;
    woff += (int64_t)layer_sizes[k] * hprev * num_fields;
    kmax = std::max(kmax, hprev * num_fields);
    hprev = layer_sizes[k];
  }
  hipStream_t st = (hipStream_t)stream;
  if (batch == 0) {  // zero gradients, nothing else to read
    hprev = num_fields;
    for (int k = 0; k < num_layers; ++k) {
      (void)hipMemsetAsync(L.dw[k], 0, sizeof(float) * (size_t)layer_sizes[k] * hprev * num_fields, st);
      if (L.dbias[k]) (void)hipMemsetAsync(L.dbias[k], 0, sizeof(float) * (size_t)layer_sizes[k], st);
      hprev = layer_sizes[k];
    }
    return check_launch("rk_cin_wgrad");
  }
  const int64_t width = (int64_t)num_fields * dim;
  if (!x0 || !maps || !dy || !aligned16(x0) || !aligned16(maps) || !aligned16(dy) || ld_x0 % 4 || ld_x0 < width)
    return fail(RK_ERR_INVALID, "rk_cin_wgrad: x0 / maps / dy must be 16-B aligned, ld_x0 %% 4 == 0, >= %lld",
                (long long)width);
  if (!workspace || workspace_floats < kCwMaxSlabs * slab_floats)
    return fail(RK_ERR_INVALID, "rk_cin_wgrad: workspace of %lld floats, needs %lld", (long long)workspace_floats,
                (long long)(kCwMaxSlabs * slab_floats));
  const int S = kCwNC / dim;
  const int64_t tiles = (batch + S - 1) / S;
  const int64_t tps = (tiles + kCwMaxSlabs - 1) / kCwMaxSlabs;
  const int64_t slabs = (tiles + tps - 1) / tps;
  const dim3 grid((unsigned)slabs, (unsigned)((kmax + kCwJB - 1) / kCwJB), (unsigned)num_layers);
  cin_wgrad_kernel<<<grid, kCbThreads, 0, st>>>(L, x0, ld_x0, num_fields, dim, hsum, batch, tiles, tps, maps, dy,
                                                workspace, slab_floats, wtot);
  cin_wgrad_reduce_kernel<<<(unsigned)((slab_floats + 255) / 256), 256, 0, st>>>(L, num_layers, num_fields, workspace,
                                                                                 slab_floats, wtot, (int)slabs);
  return check_launch("rk_cin_wgrad");
}
