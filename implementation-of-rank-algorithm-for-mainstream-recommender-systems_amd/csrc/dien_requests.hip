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
// split (one DPP row of 16 lanes per sample, 4 samples per wave, one wave per workgroup) and call
// the same DienCell code in the same order on the same values: hs is bit-equal to what
// rk_dien_interest_train writes, out / att_out to rk_dien_interest on the history replicated per
// candidate.  The fp32 h_t goes through global memory instead of LDS, which changes no bit.
// dien.hip is left as it is (its register figures are recorded in DESIGN 4a); the two passes are
// restated here rather than shared.  No atomics but the error flag, no cross-wave traffic.
#include "dien_cell.h"

namespace rk {

// Floats of LDS per sample, padded so that the four samples of a wave start 16 banks apart (their
// broadcast float4 row reads never collide), as dien_sample_stride does.
static int requests_stride(int base) {
  base += 16;
  return base + ((16 - base % 64) + 64) % 64;
}

// ---- extract: the history gather and pass 1 of dien_interest_kernel; `b` there is the request here
template <int H, int NH>
__global__ __launch_bounds__(64) void dien_extract_kernel(
    const float* __restrict__ key_table, int64_t key_rows, int64_t ld_key, const int64_t* __restrict__ seq,
    int64_t ld_seq, int64_t ld_kb, int T, const int64_t* __restrict__ seq_len, int64_t requests, const float* Wg,
    const float* bg, const float* Wc, const float* bc, int sample_stride, uint32_t* flags,
    float* __restrict__ hs_out) {
  constexpr int NG = NH / 8;
  extern __shared__ __attribute__((aligned(16))) float dien_rq_sm[];
  const int lane = threadIdx.x, p = lane & 15, s = lane >> 4, j = p % NH, half = p >> 3;
  const int64_t b = (int64_t)blockIdx.x * kDienSamples + s;
  const bool live = b < requests;
  float* rows = dien_rq_sm + (size_t)s * sample_stride;  // [T][H]: x_t
  int len = 0;
  if (live) {
    const int64_t l = seq_len[b];
    len = l < 0 ? 0 : (l > T ? T : (int)l);
  }

  // the request's len history rows into LDS: lane p resolves position t0 + p, then the 16 lanes
  // copy the 16 rows as float4 chunks (control flow is uniform over a sample's row)
  constexpr int C = H / 4;
  for (int t0 = 0; t0 < len; t0 += 16) {
    long long off = -1;
    const int t = t0 + p;
    if (t < len) {
      if (seq) {
        const int64_t r = seq[b * ld_seq + t];
        if (r >= 0 && r < key_rows)
          off = r * ld_key;
        else
          flag_oob(flags);
      } else {
        off = b * ld_kb + (int64_t)t * ld_key;
      }
    }
#pragma unroll
    for (int i = 0; i < C; ++i) {
      const int e = i * 16 + p, rr = e / C, cc = e % C;
      const long long o = __shfl(off, rr, 16);
      if (t0 + rr < len) {
        f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (o >= 0) v = *reinterpret_cast<const f32x4*>(key_table + o + 4 * cc);
        *reinterpret_cast<f32x4*>(rows + (t0 + rr) * H + 4 * cc) = v;
      }
    }
  }
  __syncthreads();

  {
    DienCell<H, NH> g;
    g.load(Wg, bg, Wc, bc, p);
    float h = 0.f, gi[NG], ci = 0.f;
#pragma unroll
    for (int i = 0; i < NG; ++i) gi[i] = 0.f;
    if (len > 0) g.input(rows, gi, ci);
    for (int t = 0; t < len; ++t) {
      float gn[NG], cn = 0.f;
#pragma unroll
      for (int i = 0; i < NG; ++i) gn[i] = 0.f;
      if (t + 1 < len) g.input(rows + (t + 1) * H, gn, cn);
      float u, c;
      g.step(gi, ci, h, half, u, c);
      h = fmaf(u, h - c, c);  // u*h + (1-u)*c
      if (p < NH) hs_out[(b * T + t) * NH + j] = h;
#pragma unroll
      for (int i = 0; i < NG; ++i) gi[i] = gn[i];
      ci = cn;
    }
  }
  if (live)
    for (int e = len * NH + p; e < T * NH; e += 16) hs_out[b * T * NH + e] = 0.f;
}

// ---- evolve: dien_interest_kernel after its first barrier, the LDS row nh wide and filled from hs
template <int H, int NH>
__global__ __launch_bounds__(64) void dien_evolve_kernel(
    const float* query, int64_t ld_query, const float* __restrict__ hs, int64_t requests, int T,
    const int64_t* __restrict__ seq_len, const int64_t* __restrict__ request_index, int64_t batch, const float* A,
    const float* Vg, const float* vg, const float* Vc, const float* vc, int cell_type, int sample_stride, float* out,
    int64_t ld_out, float* __restrict__ att_out, int64_t ld_att, uint32_t* flags) {
  constexpr int NG = NH / 8;
  extern __shared__ __attribute__((aligned(16))) float dien_rq_sm[];
  const int lane = threadIdx.x, p = lane & 15, s = lane >> 4, j = p % NH, half = p >> 3;
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
      const int64_t l = seq_len[r];
      len = l < 0 ? 0 : (l > T ? T : (int)l);
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

  // ---- A . e_target, one unit per lane
  {
    float a = 0.f;
    if (live) {
      const float* q = query + b * ld_query;
#pragma unroll
      for (int i = 0; i < H; ++i) a = fmaf(A[j * H + i], q[i], a);
    }
    if (p < NH) wea[j] = a;
  }
  __syncthreads();

  // ---- scores and the softmax over all T positions, lane p takes t = p, p + 16, ...
  {
    float wv[NH];
#pragma unroll
    for (int c4 = 0; c4 < NH / 4; ++c4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(wea + 4 * c4);
#pragma unroll
      for (int e = 0; e < 4; ++e) wv[4 * c4 + e] = v[e];
    }
    const float pad = -4294967296.0f;  // (-2**32 + 1) rounded to fp32, dien.py:216
    float m = pad;
    for (int t = p; t < T; t += 16) {
      float sc = pad;
      if (t < len) {
        sc = 0.f;
#pragma unroll
        for (int c4 = 0; c4 < NH / 4; ++c4) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(rows + t * NH + 4 * c4);
#pragma unroll
          for (int e = 0; e < 4; ++e) sc = fmaf(v[e], wv[4 * c4 + e], sc);
        }
      }
      att[t] = sc;
      m = fmaxf(m, sc);
    }
    m = row16_max(m);
    float sum = 0.f;
    for (int t = p; t < T; t += 16) {
      const float e = expf(att[t] - m);
      att[t] = e;
      sum += e;
    }
    sum = row16_sum(sum);
    const float inv = 1.0f / sum;
    for (int t = p; t < T; t += 16) {
      const float a = att[t] * inv;
      att[t] = a;
      if (att_out && live) att_out[b * ld_att + t] = a;
    }
  }
  __syncthreads();

  // ---- pass 2: interest evolution over h_t, t < len
  {
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
  if ((H != 8 && H != 16 && H != 32) || (nh != 8 && nh != 16) || T > 256)
    return fail(RK_ERR_UNSUPPORTED, "%s: H=%d nh=%d T=%d outside the envelope H in {8,16,32}, nh in {8,16}, T <= 256",
                who, H, nh, T);
  if (ld_key % 4 != 0 || ld_kb % 4 != 0 || ((uintptr_t)key_table & 15u))
    return fail(RK_ERR_UNSUPPORTED, "%s: history rows must be 16-B aligned", who);
  if (requests == 0) return RK_OK;
  const int stride = requests_stride(T * H);
  const size_t shm = (size_t)kDienSamples * stride * sizeof(float);
  const unsigned blocks = (unsigned)((requests + kDienSamples - 1) / kDienSamples);
  hipStream_t st = (hipStream_t)stream;
  uint32_t* fl = device_flags();
#define RK_DIEN_CASE(HH, NN)                                                                                  \
  if (H == HH && nh == NN) {                                                                                  \
    if (shm > 64 * 1024) raise_lds_limit((const void*)dien_extract_kernel<HH, NN>, (int)shm);                 \
    dien_extract_kernel<HH, NN><<<blocks, 64, shm, st>>>(key_table, key_rows, ld_key, seq, ld_seq, ld_kb, T,  \
                                                         seq_len, requests, Wg, bg, Wc, bc, stride, fl, hs);  \
  }
  RK_DIEN_CASE(8, 8)
  RK_DIEN_CASE(16, 8)
  RK_DIEN_CASE(32, 8)
  RK_DIEN_CASE(8, 16)
  RK_DIEN_CASE(16, 16)
  RK_DIEN_CASE(32, 16)
#undef RK_DIEN_CASE
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
  if (cell_type != 0 && cell_type != 1)
    return fail(RK_ERR_INVALID, "%s: cell_type %d is neither 0 (AGRU) nor 1 (AUGRU)", who, cell_type);
  if ((H != 8 && H != 16 && H != 32) || (nh != 8 && nh != 16) || T > 256)
    return fail(RK_ERR_UNSUPPORTED, "%s: H=%d nh=%d T=%d outside the envelope H in {8,16,32}, nh in {8,16}, T <= 256",
                who, H, nh, T);
  if ((uintptr_t)hs & 15u) return fail(RK_ERR_UNSUPPORTED, "%s: hs must be 16-B aligned", who);
  if (batch == 0 || requests == 0) return RK_OK;
  const int stride = requests_stride(T * nh + ((T + 3) & ~3));
  const size_t shm = (size_t)kDienSamples * stride * sizeof(float);
  const unsigned blocks = (unsigned)((batch + kDienSamples - 1) / kDienSamples);
  hipStream_t st = (hipStream_t)stream;
  uint32_t* fl = device_flags();
#define RK_DIEN_CASE(HH, NN)                                                                                   \
  if (H == HH && nh == NN) {                                                                                   \
    if (shm > 64 * 1024) raise_lds_limit((const void*)dien_evolve_kernel<HH, NN>, (int)shm);                   \
    dien_evolve_kernel<HH, NN><<<blocks, 64, shm, st>>>(query, ld_query, hs, requests, T, seq_len,             \
                                                        request_index, batch, A, Vg, vg, Vc, vc, cell_type,    \
                                                        stride, out, ld_out, att_out, ld_att, fl);             \
  }
  RK_DIEN_CASE(8, 8)
  RK_DIEN_CASE(16, 8)
  RK_DIEN_CASE(32, 8)
  RK_DIEN_CASE(8, 16)
  RK_DIEN_CASE(16, 16)
  RK_DIEN_CASE(32, 16)
#undef RK_DIEN_CASE
  return check_launch(who);
}
