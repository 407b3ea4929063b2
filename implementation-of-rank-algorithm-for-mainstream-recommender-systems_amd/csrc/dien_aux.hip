// DIEN auxiliary loss (DIEN/dien.py:256-300 with the paper's sign), forward and backward.  FP32.
//
// With g_t = W_aux h_t (W_aux [H, NH]), e_{t+1} the next behaviour's row and n_{t,k} the T_neg negatives
// paired with h_t (entry t * T_neg + k of the negatives):
//   aux[b] = - sum_{t < len-1} [ logsig(g_t . e_{t+1}) + sum_k logsig(-(g_t . n_{t,k})) ],  loss = mean_b aux[b]
//   logsig(x) = min(x, 0) - log1p(exp(-|x|))
// and, with k = d_loss / batch, cpos = -k sig(-pos), cneg_k = k sig(neg_k):
//   dg_t = cpos e_{t+1} + sum_k cneg_k n_{t,k};  de_{t+1} = cpos g_t;  dn_{t,k} = cneg_k g_t
//   dh_t = W_aux^T dg_t;  dW_aux = sum_{b,t} dg_t h_t^T
//
// The (b, t) items are independent and each costs 1 + T_neg random rows, one 128-B request each
// whatever H is, so the kernels are bound by gather requests, not arithmetic.  Work split: one wave
// per sample, H / 4 lanes per item (one float4 of every row per lane), 64 / (H / 4) items in flight
// per wave.  A lane's float4 slot is fixed, so the four rows of W_aux it needs for its part of g_t
// live in registers for the whole kernel (4 NH values, read once; W_aux is at most 512 floats).  Per
// item every index load is issued before the first row load and every row load before the first
// dot; the dots are summed over the item's lanes on DPP.  The per-sample sum runs over each lane's
// items in t order and then over the wave by a fixed butterfly, the mean is one wave over
// per_sample in a fixed order: no float atomics, two calls are bit-equal.
//
// The backward recomputes the dots (1 + T_neg floats per step would cost more to save than to redo)
// and writes dg rows [batch * T, H] to the workspace, rows t >= len-1 zero; dh = dg W_aux is one
// rk_gemm and dW_aux = dg^T hs one rk_gemm_wgrad over those rows.
#include "common.h"

namespace rk {

constexpr int kAuxMaxNeg = 8;
constexpr int kAuxWaves = 4;  // samples (= waves) per workgroup

// Where the history rows and the negatives' rows come from: tables with ids (seq / neg_seq set), or
// dense tensors (both null).
struct AuxSrc {
  const float* keys;       // table [key_rows, ld_key] or dense [batch, T, .]: row t at b * ld_kb + t * ld_key
  const float* neg;        // table (= keys' table) or dense [batch, (T-1) T_neg, .]: row i at b * ld_nb + i * ld_neg
  const int64_t* seq;      // [batch, ld_seq] or null
  const int64_t* neg_seq;  // [batch, ld_nseq] or null
  int64_t key_rows, ld_key, ld_seq, ld_kb, ld_neg, ld_nseq, ld_nb;
};

__device__ __forceinline__ float log_sigmoid(float x) { return fminf(x, 0.f) - log1pf(expf(-fabsf(x))); }

// Sum over the H / 4 lanes of an item (2, 4 or 8 lanes, aligned inside a DPP row); every lane of the
// item ends with the same bits.
template <int L>
__device__ __forceinline__ float item_sum(float v) {
  v += dpp_f32<0xB1>(v);                          // quad_perm [1,0,3,2]
  if constexpr (L >= 4) v += dpp_f32<0x4E>(v);    // quad_perm [2,3,0,1]
  if constexpr (L >= 8) v += dpp_f32<0x141>(v);   // row_half_mirror
  return v;
}

__device__ __forceinline__ float dot4(f32x4 a, f32x4 b) {
  return fmaf(a[3], b[3], fmaf(a[2], b[2], fmaf(a[1], b[1], a[0] * b[0])));
}

// One item's rows and dots as lane `sub` of the item sees them.
template <int H, int NH>
struct AuxItem {
  int64_t ids[1 + kAuxMaxNeg];
  f32x4 e[1 + kAuxMaxNeg];  // this lane's float4 of e_{t+1} and of the negatives
  f32x4 g;                  // this lane's float4 of g_t
  float dot[1 + kAuxMaxNeg];

  // FLAG: an out-of-range id raises RK_FLAG_INDEX_OOB (the forward); it reads a zero row either way.
  template <bool FLAG>
  __device__ __forceinline__ void load(const AuxSrc& s, int64_t b, int t, int tneg, int sub, const float* hsb,
                                       const float (&w)[4][NH], uint32_t* flags) {
    const bool gather = s.seq != nullptr;
    if (gather) {  // every index load first
      ids[0] = s.seq[b * s.ld_seq + t + 1];
#pragma unroll
      for (int n = 0; n < kAuxMaxNeg; ++n)
        if (n < tneg) ids[1 + n] = s.neg_seq[b * s.ld_nseq + (int64_t)t * tneg + n];
    }
    const float* row[1 + kAuxMaxNeg];
    if (gather) {
      row[0] = ids[0] >= 0 && ids[0] < s.key_rows ? s.keys + ids[0] * s.ld_key : nullptr;
#pragma unroll
      for (int n = 0; n < kAuxMaxNeg; ++n)
        if (n < tneg) row[1 + n] = ids[1 + n] >= 0 && ids[1 + n] < s.key_rows ? s.neg + ids[1 + n] * s.ld_neg : nullptr;
    } else {
      row[0] = s.keys + b * s.ld_kb + (int64_t)(t + 1) * s.ld_key;
#pragma unroll
      for (int n = 0; n < kAuxMaxNeg; ++n)
        if (n < tneg) row[1 + n] = s.neg + b * s.ld_nb + ((int64_t)t * tneg + n) * s.ld_neg;
    }
    // then every row load: h_t and this lane's float4 of the 1 + T_neg rows
    f32x4 h[NH / 4];
#pragma unroll
    for (int c = 0; c < NH / 4; ++c) h[c] = *reinterpret_cast<const f32x4*>(hsb + (int64_t)t * NH + 4 * c);
    const f32x4 zero = (f32x4){0.f, 0.f, 0.f, 0.f};
    e[0] = row[0] ? *reinterpret_cast<const f32x4*>(row[0] + 4 * sub) : zero;
#pragma unroll
    for (int n = 0; n < kAuxMaxNeg; ++n)
      if (n < tneg) e[1 + n] = row[1 + n] ? *reinterpret_cast<const f32x4*>(row[1 + n] + 4 * sub) : zero;
    if constexpr (FLAG) {
      bool bad = !row[0];
#pragma unroll
      for (int n = 0; n < kAuxMaxNeg; ++n)
        if (n < tneg) bad |= !row[1 + n];
      if (bad && sub == 0) flag_oob(flags);
    }
    // g_t = W_aux h_t (rows 4 sub ... 4 sub + 3), then the dots
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float a = 0.f;
#pragma unroll
      for (int j = 0; j < NH; ++j) a = fmaf(w[i][j], h[j / 4][j % 4], a);
      g[i] = a;
    }
    dot[0] = item_sum<H / 4>(dot4(g, e[0]));
#pragma unroll
    for (int n = 0; n < kAuxMaxNeg; ++n)
      if (n < tneg) dot[1 + n] = item_sum<H / 4>(dot4(g, e[1 + n]));
  }
};

template <int NH>
__device__ __forceinline__ void aux_load_w(const float* W, int sub, float (&w)[4][NH]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NH; ++j) w[i][j] = W[(4 * sub + i) * NH + j];
}

__device__ __forceinline__ int aux_len(const int64_t* seq_len, int64_t b, int T) {
  const int64_t l = seq_len[b];
  return l < 0 ? 0 : (l > T ? T : (int)l);
}

template <int H, int NH>
__global__ __launch_bounds__(64 * kAuxWaves) void dien_aux_loss_kernel(
    AuxSrc src, const float* __restrict__ hs, const float* __restrict__ W, int T, int tneg,
    const int64_t* __restrict__ seq_len, int64_t batch, float* __restrict__ per_sample, uint32_t* flags) {
  constexpr int L = H / 4, G = kWave / L;
  const int lane = threadIdx.x & 63, sub = lane % L, grp = lane / L;
  const int64_t b = (int64_t)blockIdx.x * kAuxWaves + wave_id();
  if (b >= batch) return;  // no barrier below: a wave past the batch just leaves
  const int len = aux_len(seq_len, b, T);
  float w[4][NH];
  aux_load_w<NH>(W, sub, w);
  const float* hsb = hs + b * T * NH;
  float acc = 0.f;
  for (int t = grp; t < len - 1; t += G) {
    AuxItem<H, NH> it;
    it.template load<true>(src, b, t, tneg, sub, hsb, w, flags);
    float v = log_sigmoid(it.dot[0]);
#pragma unroll
    for (int n = 0; n < kAuxMaxNeg; ++n)
      if (n < tneg) v += log_sigmoid(-it.dot[1 + n]);
    acc += v;
  }
  const float total = wave_sum(sub == 0 ? acc : 0.f);
  if (lane == 0) per_sample[b] = 0.f - total;  // +0 for a sample without a term
}

template <int H, int NH>
__global__ __launch_bounds__(64 * kAuxWaves) void dien_aux_loss_backward_kernel(
    AuxSrc src, const float* __restrict__ hs, const float* __restrict__ W, int T, int tneg,
    const int64_t* __restrict__ seq_len, int64_t batch, const float* __restrict__ d_loss, float* __restrict__ dg,
    float* __restrict__ dkeys, float* __restrict__ dneg, int64_t* __restrict__ seq_masked,
    int64_t* __restrict__ neg_masked) {
  constexpr int L = H / 4, G = kWave / L;
  const int lane = threadIdx.x & 63, sub = lane % L, grp = lane / L;
  const int64_t b = (int64_t)blockIdx.x * kAuxWaves + wave_id();
  if (b >= batch) return;
  const int len = aux_len(seq_len, b, T);
  const float k = d_loss[0] / (float)batch;
  float w[4][NH];
  aux_load_w<NH>(W, sub, w);
  const float* hsb = hs + b * T * NH;
  const f32x4 zero = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int64_t nrow0 = b * (int64_t)(T - 1) * tneg;  // this sample's first row of dneg / neg_masked
  // every t < T: steps past len-1 write the zero rows (dg row t, dkeys row t+1, dneg rows of t)
  for (int t = grp; t < T; t += G) {
    const int64_t nrow = nrow0 + (int64_t)t * tneg;
    if (t == 0) {
      *reinterpret_cast<f32x4*>(dkeys + b * T * H + 4 * sub) = zero;
      if (seq_masked && sub == 0) seq_masked[b * T] = 0;
    }
    if (t < len - 1) {  // a live step (so t + 1 < T)
      AuxItem<H, NH> it;
      it.template load<false>(src, b, t, tneg, sub, hsb, w, nullptr);
      const float cpos = -k / (1.0f + expf(it.dot[0]));  // -k sig(-pos)
      f32x4 dgt = cpos * it.e[0];
      *reinterpret_cast<f32x4*>(dkeys + (b * T + t + 1) * H + 4 * sub) = cpos * it.g;
      if (seq_masked && sub == 0) seq_masked[b * T + t + 1] = it.ids[0];
#pragma unroll
      for (int n = 0; n < kAuxMaxNeg; ++n)
        if (n < tneg) {
          const float cneg = k / (1.0f + expf(-it.dot[1 + n]));  // k sig(neg)
          dgt += cneg * it.e[1 + n];
          *reinterpret_cast<f32x4*>(dneg + (nrow + n) * H + 4 * sub) = cneg * it.g;
          if (neg_masked && sub == 0) neg_masked[nrow + n] = it.ids[1 + n];
        }
      *reinterpret_cast<f32x4*>(dg + (b * T + t) * H + 4 * sub) = dgt;
    } else {
      *reinterpret_cast<f32x4*>(dg + (b * T + t) * H + 4 * sub) = zero;
      if (t + 1 < T) {
        *reinterpret_cast<f32x4*>(dkeys + (b * T + t + 1) * H + 4 * sub) = zero;
        if (seq_masked && sub == 0) seq_masked[b * T + t + 1] = 0;
        for (int n = 0; n < tneg; ++n) {
          *reinterpret_cast<f32x4*>(dneg + (nrow + n) * H + 4 * sub) = zero;
          if (neg_masked && sub == 0) neg_masked[nrow + n] = 0;
        }
      }
    }
  }
}

static int64_t aux_align4(int64_t n) { return (n + 3) & ~(int64_t)3; }

static int aux_check(const char* who, int32_t T, int32_t T_neg, int64_t batch, int32_t H, int32_t nh) {
  if (T <= 0 || T_neg <= 0 || batch < 0 || H <= 0 || nh <= 0)
    return fail(RK_ERR_INVALID, "%s: bad shape T=%d T_neg=%d H=%d nh=%d", who, T, T_neg, H, nh);
  if ((H != 8 && H != 16 && H != 32) || (nh != 8 && nh != 16) || T > 256 || T_neg > kAuxMaxNeg)
    return fail(RK_ERR_UNSUPPORTED,
                "%s: H=%d nh=%d T=%d T_neg=%d outside the envelope H in {8,16,32}, nh in {8,16}, T <= 256, "
                "T_neg <= 8", who, H, nh, T, T_neg);
  if (batch > INT32_MAX) return fail(RK_ERR_UNSUPPORTED, "%s: batch too large", who);
  return RK_OK;
}

static int aux_forward(const char* who, const AuxSrc& src, const float* hs, const float* W_aux, int32_t T,
                       int32_t T_neg, const int64_t* seq_len, int64_t batch, int32_t H, int32_t nh,
                       float* per_sample, float* mean, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (batch == 0) {
    (void)hipMemsetAsync(mean, 0, sizeof(float), st);
    return check_launch(who);
  }
  const unsigned blocks = (unsigned)((batch + kAuxWaves - 1) / kAuxWaves);
  uint32_t* fl = device_flags();
#define RK_AUX_CASE(HH, NN)                                                                                    \
  if (H == HH && nh == NN)                                                                                     \
    dien_aux_loss_kernel<HH, NN><<<blocks, 64 * kAuxWaves, 0, st>>>(src, hs, W_aux, T, T_neg, seq_len, batch,  \
                                                                    per_sample, fl);
  RK_AUX_CASE(8, 8)
  RK_AUX_CASE(16, 8)
  RK_AUX_CASE(32, 8)
  RK_AUX_CASE(8, 16)
  RK_AUX_CASE(16, 16)
  RK_AUX_CASE(32, 16)
#undef RK_AUX_CASE
  const int rc = check_launch(who);
  if (rc != RK_OK) return rc;
  return launch_l2_final(per_sample, (int)batch, batch, 1.0f, mean, st);  // mean_b aux[b], one wave, fixed order
}

}  // namespace rk

using namespace rk;

RK_API int rk_dien_aux_loss(const float* hs, const float* key_table, int64_t key_rows, int64_t ld_key,
                            const int64_t* seq, int64_t ld_seq, const int64_t* neg_seq, int64_t ld_neg_seq, int32_t T,
                            int32_t T_neg, const int64_t* seq_len, int64_t batch, int32_t H, int32_t nh,
                            const float* W_aux, float* per_sample, float* mean, void* stream) {
  const char* who = "rk_dien_aux_loss";
  if (!hs || !key_table || !seq || !seq_len || !W_aux || !per_sample || !mean || (T > 1 && !neg_seq))
    return fail(RK_ERR_INVALID, "%s: null pointer", who);
  int rc = aux_check(who, T, T_neg, batch, H, nh);
  if (rc != RK_OK) return rc;
  if (key_rows <= 0 || ld_key < H || ld_seq < T || ld_neg_seq < (int64_t)(T - 1) * T_neg)
    return fail(RK_ERR_INVALID, "%s: bad table / id strides", who);
  if (ld_key % 4 != 0 || (((uintptr_t)key_table | (uintptr_t)hs) & 15u))
    return fail(RK_ERR_UNSUPPORTED, "%s: table rows and hs must be 16-B aligned", who);
  const AuxSrc src{key_table, key_table, seq, neg_seq, key_rows, ld_key, ld_seq, 0, ld_key, ld_neg_seq, 0};
  return aux_forward(who, src, hs, W_aux, T, T_neg, seq_len, batch, H, nh, per_sample, mean, stream);
}

RK_API int rk_dien_aux_loss_dense(const float* hs, const float* keys, int64_t ld_keys_b, int64_t ld_keys_t,
                                  const float* neg, int64_t ld_neg_b, int64_t ld_neg_r, int32_t T, int32_t T_neg,
                                  const int64_t* seq_len, int64_t batch, int32_t H, int32_t nh, const float* W_aux,
                                  float* per_sample, float* mean, void* stream) {
  const char* who = "rk_dien_aux_loss_dense";
  if (!hs || !keys || !seq_len || !W_aux || !per_sample || !mean || (T > 1 && !neg))
    return fail(RK_ERR_INVALID, "%s: null pointer", who);
  int rc = aux_check(who, T, T_neg, batch, H, nh);
  if (rc != RK_OK) return rc;
  if (ld_keys_t < H || ld_neg_r < H || (batch > 1 && (ld_keys_b < (int64_t)T * ld_keys_t ||
                                                     ld_neg_b < (int64_t)(T - 1) * T_neg * ld_neg_r)))
    return fail(RK_ERR_INVALID, "%s: bad strides", who);
  if (ld_keys_t % 4 != 0 || ld_keys_b % 4 != 0 || ld_neg_r % 4 != 0 || ld_neg_b % 4 != 0 ||
      (((uintptr_t)keys | (uintptr_t)neg | (uintptr_t)hs) & 15u))
    return fail(RK_ERR_UNSUPPORTED, "%s: history rows, negative rows and hs must be 16-B aligned", who);
  const AuxSrc src{keys, neg, nullptr, nullptr, 0, ld_keys_t, 0, ld_keys_b, ld_neg_r, 0, ld_neg_b};
  return aux_forward(who, src, hs, W_aux, T, T_neg, seq_len, batch, H, nh, per_sample, mean, stream);
}

RK_API int64_t rk_dien_aux_loss_backward_workspace_floats(int64_t batch, int32_t T, int32_t H, int32_t nh) {
  if (batch <= 0 || T <= 0 || H <= 0 || nh <= 0) return 0;
  const int64_t R = batch * T;
  return aux_align4(R * H) + aux_align4(rk_gemm_wgrad_workspace_floats(H, nh, R));
}

RK_API int rk_dien_aux_loss_backward(const float* hs, const float* keys, int64_t key_rows, int64_t ld_key,
                                     const int64_t* seq, int64_t ld_seq, int64_t ld_keys_b, const float* neg,
                                     int64_t ld_neg_b, int64_t ld_neg_r, const int64_t* neg_seq, int64_t ld_neg_seq,
                                     int32_t T, int32_t T_neg, const int64_t* seq_len, int64_t batch, int32_t H,
                                     int32_t nh, const float* W_aux, const float* d_loss, float* d_hs, float* dkeys,
                                     float* dneg, int64_t* seq_masked, int64_t* neg_masked, float* dW_aux,
                                     float* workspace,
                                     int64_t workspace_floats, void* stream) {
  const char* who = "rk_dien_aux_loss_backward";
  if (!hs || !keys || !seq_len || !W_aux || !d_loss || !d_hs || !dkeys || !dW_aux || (T > 1 && !dneg))
    return fail(RK_ERR_INVALID, "%s: null pointer", who);
  int rc = aux_check(who, T, T_neg, batch, H, nh);
  if (rc != RK_OK) return rc;
  const bool gather = seq != nullptr;
  const int64_t nneg = (int64_t)(T - 1) * T_neg;
  if (gather) {
    if ((T > 1 && !neg_seq) || key_rows <= 0 || ld_key < H || ld_seq < T || ld_neg_seq < nneg)
      return fail(RK_ERR_INVALID, "%s: bad table / id strides", who);
    if (ld_key % 4 != 0) return fail(RK_ERR_UNSUPPORTED, "%s: table rows must be 16-B aligned", who);
  } else {
    if ((T > 1 && !neg) || neg_seq || seq_masked || neg_masked || ld_key < H || ld_neg_r < H ||
        (batch > 1 && (ld_keys_b < (int64_t)T * ld_key || ld_neg_b < nneg * ld_neg_r)))
      return fail(RK_ERR_INVALID, "%s: bad dense strides", who);
    if (ld_key % 4 != 0 || ld_keys_b % 4 != 0 || ld_neg_r % 4 != 0 || ld_neg_b % 4 != 0 || ((uintptr_t)neg & 15u))
      return fail(RK_ERR_UNSUPPORTED, "%s: history and negative rows must be 16-B aligned", who);
  }
  if ((((uintptr_t)keys | (uintptr_t)hs | (uintptr_t)dkeys | (uintptr_t)dneg | (uintptr_t)d_hs | (uintptr_t)dW_aux) & 15u))
    return fail(RK_ERR_UNSUPPORTED, "%s: rows, hs and the gradient buffers must be 16-B aligned", who);
  hipStream_t st = (hipStream_t)stream;
  if (batch == 0) {
    (void)hipMemsetAsync(dW_aux, 0, sizeof(float) * H * nh, st);
    return check_launch(who);
  }
  const int64_t R = batch * T;
  const int64_t need = rk_dien_aux_loss_backward_workspace_floats(batch, T, H, nh);
  if (!workspace || ((uintptr_t)workspace & 15u) || workspace_floats < need)
    return fail(RK_ERR_INVALID, "%s: needs a 16-B aligned workspace of %lld floats, got %lld", who, (long long)need,
                (long long)workspace_floats);
  float* dg = workspace;
  float* ws = workspace + aux_align4(R * H);
  const int64_t nws = need - aux_align4(R * H);
  const AuxSrc src = gather ? AuxSrc{keys, keys, seq, neg_seq, key_rows, ld_key, ld_seq, 0, ld_key, ld_neg_seq, 0}
                            : AuxSrc{keys, neg, nullptr, nullptr, 0, ld_key, 0, ld_keys_b, ld_neg_r, 0, ld_neg_b};
  const unsigned blocks = (unsigned)((batch + kAuxWaves - 1) / kAuxWaves);
#define RK_AUX_CASE(HH, NN)                                                                                      \
  if (H == HH && nh == NN)                                                                                       \
    dien_aux_loss_backward_kernel<HH, NN><<<blocks, 64 * kAuxWaves, 0, st>>>(src, hs, W_aux, T, T_neg, seq_len,  \
                                                                             batch, d_loss, dg, dkeys, dneg,     \
                                                                             seq_masked, neg_masked);
  RK_AUX_CASE(8, 8)
  RK_AUX_CASE(16, 8)
  RK_AUX_CASE(32, 8)
  RK_AUX_CASE(8, 16)
  RK_AUX_CASE(16, 16)
  RK_AUX_CASE(32, 16)
#undef RK_AUX_CASE
  if ((rc = check_launch(who)) != RK_OK) return rc;
  // dh = dg W_aux (rows t >= len-1 of dg are zero, so are those of d_hs); dW_aux = dg^T hs
  if ((rc = rk_gemm(0, 1, R, nh, H, dg, H, nullptr, W_aux, nh, d_hs, nh, nullptr, 0, 1, stream)) != RK_OK) return rc;
  return rk_gemm_wgrad(H, nh, R, dg, H, nullptr, hs, nh, dW_aux, nh, nullptr, 0, ws, nws, stream);
}
