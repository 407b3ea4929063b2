// DIEN request-level scoring: dien_interest_kernel (dien.hip) cut at its first barrier into two
// launches, for a ranking request of one behaviour history and N candidates.
//
//   extract  per request r:   h_t = GRUCell(x_t, h_{t-1}), t < len[r]  ->  hs [R, T, nh], rows t >= len zero
//   evolve   per candidate b: r = request_index[b]; attention of hs[r] against A e_target(b), masked
//            softmax over all T, AGRU / AUGRU over h_t, t < len[r]      ->  out[b], att_out[b]
//
// Pass 1 of the fused kernel never reads the query, so the N candidates of a request share one
// extraction (and one history gather); hs depends on the history and the weights only, so a server
// may keep it per user for as long as the weights stand.  Both kernels keep the fused kernel's work
// split (one DPP row of 16 lanes per sample, 4 samples per wave, one wave per workgroup) and are made
// of the fused kernel's own phases (dien_cell.h), instantiated for another LDS row width (evolve
// restates pass 2 alone, and says why): hs is bit-equal to what rk_dien_interest_train writes, out /
// att_out to rk_dien_interest on the history replicated per candidate.  The fp32 h_t goes through
// global memory instead of LDS, which changes no bit.  No atomics but the error flag, no cross-wave
// traffic.
#include "dien_cell.h"

namespace rk {

// ---- extract: the history gather and pass 1; the LDS row is H wide and h_t goes to hs_out only
template <int H, int NH>
__global__ __launch_bounds__(64) void dien_extract_kernel(
    const float* __restrict__ key_table, int64_t key_rows, int64_t ld_key, const int64_t* __restrict__ seq,
    int64_t ld_seq, int64_t ld_kb, int T, const int64_t* __restrict__ seq_len, int64_t requests, const float* Wg,
    const float* bg, const float* Wc, const float* bc, int sample_stride, uint32_t* flags,
    float* __restrict__ hs_out) {
  extern __shared__ __attribute__((aligned(16))) float dien_rq_sm[];
  const int lane = threadIdx.x, p = lane & 15, s = lane >> 4;
  const int64_t b = (int64_t)blockIdx.x * kDienSamples + s;  // the request
  const bool live = b < requests;
  float* rows = dien_rq_sm + (size_t)s * sample_stride;  // [T][H]: x_t
  const int len = live ? dien_len(seq_len, b, T) : 0;

  dien_gather_rows<H, H>(key_table, key_rows, ld_key, seq, ld_seq, ld_kb, b, len, p, flags, rows);
  __syncthreads();
  dien_extract_pass<H, NH, H, false, true>(Wg, bg, Wc, bc, rows, len, p, hs_out, b, T);
  if (live)
    for (int e = len * NH + p; e < T * NH; e += 16) hs_out[b * T * NH + e] = 0.f;
}

// ---- evolve: the fused kernel after its first barrier, the LDS row nh wide and filled from hs
template <int H, int NH>
__global__ __launch_bounds__(64) void dien_evolve_kernel(
    const float* query, int64_t ld_query, const float* __restrict__ hs, int64_t requests, int T,
    const int64_t* __restrict__ seq_len, const int64_t* __restrict__ request_index, int64_t batch, const float* A,
    const float* Vg, const float* vg, const float* Vc, const float* vc, int cell_type, int sample_stride, float* out,
    int64_t ld_out, float* __restrict__ att_out, int64_t ld_att, uint32_t* flags) {
  extern __shared__ __attribute__((aligned(16))) float dien_rq_sm[];
  const int lane = threadIdx.x, p = lane & 15, s = lane >> 4;
  const int64_t b = (int64_t)blockIdx.x * kDienSamples + s;
  const bool live = b < batch;
  float* rows = dien_rq_sm + (size_t)s * sample_stride;  // [T][NH]: h_t
  float* att = rows + T * NH;                             // [T]: scores, then attention weights
  float* wea = att + ((T + 3) & ~3);                      // [NH]: A . e_target
  int len = 0;
  int64_t r = 0;
  if (live) {
    r = request_index[b];
    if (r >= 0 && r < requests) {
      len = dien_len(seq_len, r, T);
    } else {  // no such request: an empty history (zero state, uniform attention)
      if (p == 0) flag_oob(flags);
      r = 0;
    }
  }

  // rows t < len of hs[r] are contiguous: float4 chunks over the 16 lanes
  {
    const f32x4* src = reinterpret_cast<const f32x4*>(hs + r * T * NH);
    f32x4* dst = reinterpret_cast<f32x4*>(rows);
    for (int e = p; e < len * (NH / 4); e += 16) dst[e] = src[e];
  }
  dien_project_query<H, NH>(A, query, ld_query, b, live, p, wea);
  __syncthreads();
  dien_attention<NH, NH>(rows, wea, att, T, len, p, att_out, ld_att, b, live);
  __syncthreads();
  // Pass 2 is dien_evolve_pass<NH, NH, false>, restated: called, the same instructions come out with one
  // s_waitcnt of the loop a slot later, and evolve alone measured 0.3-0.5 % slower at B 32768.
  {
    constexpr int NG = NH / 8;
    const int j = p % NH, half = p >> 3;
    DienCell<NH, NH> g;
    g.load(Vg, vg, Vc, vc, p);
    float st = 0.f, gi[NG], ci = 0.f, a = 0.f;
#pragma unroll
    for (int i = 0; i < NG; ++i) gi[i] = 0.f;
    if (len > 0) {
      g.input(rows, gi, ci);
      a = att[0];
    }
    for (int t = 0; t < len; ++t) {
      float gn[NG], cn = 0.f, an = 0.f;
#pragma unroll
      for (int i = 0; i < NG; ++i) gn[i] = 0.f;
      if (t + 1 < len) {
        g.input(rows + (t + 1) * NH, gn, cn);
        an = att[t + 1];
      }
      float u, c;
      g.step(gi, ci, st, half, u, c);
      if (cell_type == 0) {
        st = fmaf(a, c - st, st);  // (1-a)*s + a*c
      } else {
        const float u2 = fmaf(-a, u, u);  // (1-a)*u
        st = fmaf(u2, st - c, c);         // u'*s + (1-u')*c
      }
#pragma unroll
      for (int i = 0; i < NG; ++i) gi[i] = gn[i];
      ci = cn;
      a = an;
    }
    if (live && p < NH) out[b * ld_out + j] = st;
  }
}

}  // namespace rk

using namespace rk;

static int launch_extract(const float* key_table, int64_t key_rows, int64_t ld_key, const int64_t* seq, int64_t ld_seq,
                          int64_t ld_kb, int32_t T, const int64_t* seq_len, int64_t requests, int32_t H, int32_t nh,
                          const float* Wg, const float* bg, const float* Wc, const float* bc, float* hs, void* stream,
                          const char* who) {
  if (!key_table || !seq_len || !Wg || !bg || !Wc || !bc || !hs) return fail(RK_ERR_INVALID, "%s: null pointer", who);
  if (T <= 0 || requests < 0 || H <= 0 || nh <= 0 || ld_key < H)
    return fail(RK_ERR_INVALID, "%s: bad shape T=%d H=%d nh=%d", who, T, H, nh);
  if (int rc = dien_check_envelope(who, H, nh, T)) return rc;
  if (int rc = dien_check_history_rows(who, key_table, ld_key, ld_kb)) return rc;
  if (requests == 0) return RK_OK;
  const int stride = dien_padded_stride(T * H + 16);
  const size_t shm = (size_t)kDienSamples * stride * sizeof(float);
  const unsigned blocks = (unsigned)((requests + kDienSamples - 1) / kDienSamples);
  dien_launch(
      H, nh, [](auto s) { return dien_extract_kernel<s.H, s.NH>; }, blocks, shm, (hipStream_t)stream, key_table,
      key_rows, ld_key, seq, ld_seq, ld_kb, T, seq_len, requests, Wg, bg, Wc, bc, stride, device_flags(), hs);
  return check_launch(who);
}

RK_API int rk_dien_extract(const float* key_table, int64_t key_rows, int64_t ld_key, const int64_t* seq,
                           int64_t ld_seq, int32_t T, const int64_t* seq_len, int64_t requests, int32_t H,
                           int32_t nh, const float* Wg, const float* bg, const float* Wc, const float* bc, float* hs,
                           void* stream) {
  if (!seq) return fail(RK_ERR_INVALID, "rk_dien_extract: null pointer");
  if (key_rows <= 0 || ld_seq < T) return fail(RK_ERR_INVALID, "rk_dien_extract: bad shape T=%d", T);
  return launch_extract(key_table, key_rows, ld_key, seq, ld_seq, 0, T, seq_len, requests, H, nh, Wg, bg, Wc, bc, hs,
                        stream, "rk_dien_extract");
}

RK_API int rk_dien_extract_dense(const float* keys, int64_t ld_keys_b, int64_t ld_keys_t, int32_t T,
                                 const int64_t* keys_length, int64_t requests, int32_t H, int32_t nh,
                                 const float* Wg, const float* bg, const float* Wc, const float* bc, float* hs,
                                 void* stream) {
  if (T > 0 && ld_keys_b < (int64_t)T * ld_keys_t && requests > 1)
    return fail(RK_ERR_INVALID, "rk_dien_extract_dense: bad shape T=%d", T);
  return launch_extract(keys, 0, ld_keys_t, nullptr, 0, ld_keys_b, T, keys_length, requests, H, nh, Wg, bg, Wc, bc,
                        hs, stream, "rk_dien_extract_dense");
}

RK_API int rk_dien_evolve(const float* query, int64_t ld_query, const float* hs, int64_t requests, int32_t T,
                          const int64_t* seq_len, const int64_t* request_index, int64_t batch, int32_t H, int32_t nh,
                          int32_t cell_type, const float* A, const float* Vg, const float* vg, const float* Vc,
                          const float* vc, float* out, int64_t ld_out, float* att_out, int64_t ld_att,
                          void* stream) {
  const char* who = "rk_dien_evolve";
  if (!query || !hs || !seq_len || !request_index || !A || !Vg || !vg || !Vc || !vc || !out)
    return fail(RK_ERR_INVALID, "%s: null pointer", who);
  if (T <= 0 || batch < 0 || requests < 0 || H <= 0 || nh <= 0 || ld_query < H || ld_out < nh ||
      (att_out && ld_att < T))
    return fail(RK_ERR_INVALID, "%s: bad shape T=%d H=%d nh=%d", who, T, H, nh);
  if (int rc = dien_check_cell(who, cell_type)) return rc;
  if (int rc = dien_check_envelope(who, H, nh, T)) return rc;
  if ((uintptr_t)hs & 15u) return fail(RK_ERR_UNSUPPORTED, "%s: hs must be 16-B aligned", who);
  if (batch == 0 || requests == 0) return RK_OK;
  const int stride = dien_padded_stride(T * nh + ((T + 3) & ~3) + 16);
  const size_t shm = (size_t)kDienSamples * stride * sizeof(float);
  const unsigned blocks = (unsigned)((batch + kDienSamples - 1) / kDienSamples);
  dien_launch(
      H, nh, [](auto s) { return dien_evolve_kernel<s.H, s.NH>; }, blocks, shm, (hipStream_t)stream, query, ld_query,
      hs, requests, T, seq_len, request_index, batch, A, Vg, vg, Vc, vc, cell_type, stride, out, ld_out, att_out,
      ld_att, device_flags());
  return check_launch(who);
}
