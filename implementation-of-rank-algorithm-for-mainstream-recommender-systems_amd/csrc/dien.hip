// DIEN interest extractor + interest evolution (reference: dien.py:198-229, custom_grucell.py:19-167,
// rnn.py:201-219), eval forward, FP32, one launch.
//
//   GRU (TF GRUCell, h_-1 = 0):   [r|u] = sigmoid([x_t, h] Wg^T + bg);  c = tanh([x_t, r*h] Wc^T + bc)
//                                 h_t = u*h + (1-u)*c
//   attention:                    s_t = h_t . (A e_target),  s_t = -2^32+1 for t >= len,  a = softmax_T(s)
//   evolution (s_-1 = 0, t < len, input h_t, weights Vg / Vc):
//       AGRU:   s = (1-a_t)*s + a_t*c          AUGRU:  u' = (1-a_t)*u;  s = u'*s + (1-u')*c
//   out = s after step len-1 (zero when len = 0)
//
// Work split: one DPP row (16 lanes) per sample, 4 samples per wave, one wave per workgroup, so
// batch 4096 is 1024 waves.  The kernel is a dependent chain of 2*len steps; what a step costs is
// its instruction count, so the state never leaves registers: lane p holds the state of unit
// p % nh, and the state halves of both mat-vecs are nh FMAs over the row rotated with row_ror DPP
// moves (each lane's weights are loaded in the order the rotations deliver the units).  nh = 8: lane
// p computes gate row p (r in lanes 0-7, u in lanes 8-15, swapped across by one row_ror:8) and both
// halves keep a copy of the state; nh = 16: lane p computes r_p and u_p.  The input halves
// (x_t . Wg[:, :H], x_t . Wc[:, :H]) do not depend on the state: they are computed one step ahead
// from LDS, where the sample's len history rows are gathered up front (ids at t >= len are never
// read).  h_t overwrites row t of that buffer, the scores and the softmax run over it once the
// first pass is done, and the second pass reads h_t and a_t back one step ahead again.
// No cross-wave traffic, no atomics: results are bit-reproducible, and the table form and the
// dense form run the same code after the gather.
#include "dien_cell.h"

namespace rk {

// SAVE (the train forward): the extractor states h_t, the evolution states s_t and the attention
// weights also go to hs_out / ss_out [batch, T, NH] (rows t >= len zero) and att_out for the
// backward (dien_train.hip).  The arithmetic is the eval kernel's, so the state is bit-equal.
template <int H, int NH, bool SAVE>
__global__ __launch_bounds__(64) void dien_interest_kernel(
    const float* query, int64_t ld_query, const float* __restrict__ key_table, int64_t key_rows, int64_t ld_key,
    const int64_t* __restrict__ seq, int64_t ld_seq, int64_t ld_kb, int T, const int64_t* __restrict__ seq_len,
    int64_t batch, DienWeights w, int cell_type, int sample_stride, float* out, int64_t ld_out,
    float* __restrict__ att_out, int64_t ld_att, uint32_t* flags, float* __restrict__ hs_out,
    float* __restrict__ ss_out) {
  constexpr int RW = H > NH ? H : NH;  // LDS row: x_t first, h_t after step t
  constexpr int NG = NH / 8;
  extern __shared__ __attribute__((aligned(16))) float dien_sm[];
  const int lane = threadIdx.x, p = lane & 15, s = lane >> 4, j = p % NH, half = p >> 3;
  const int64_t b = (int64_t)blockIdx.x * kDienSamples + s;
  const bool live = b < batch;
  float* rows = dien_sm + (size_t)s * sample_stride;  // [T][RW]
  float* att = rows + T * RW;                          // [T]: scores, then attention weights
  float* wea = att + ((T + 3) & ~3);                   // [NH]: A . e_target
  int len = 0;
  if (live) {
    const int64_t l = seq_len[b];
    len = l < 0 ? 0 : (l > T ? T : (int)l);
  }

  // ---- the sample's len history rows into LDS: lane p resolves position t0 + p, then the 16
  // lanes copy the 16 rows as float4 chunks (control flow is uniform over a sample's row)
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
        *reinterpret_cast<f32x4*>(rows + (t0 + rr) * RW + 4 * cc) = v;
      }
    }
  }

  // ---- A . e_target, one unit per lane
  {
    float a = 0.f;
    if (live) {
      const float* q = query + b * ld_query;
#pragma unroll
      for (int i = 0; i < H; ++i) a = fmaf(w.A[j * H + i], q[i], a);
    }
    if (p < NH) wea[j] = a;
  }
  __syncthreads();

  // ---- pass 1: interest extractor
  {
    DienCell<H, NH> g;
    g.load(w.Wg, w.bg, w.Wc, w.bc, p);
    float h = 0.f, gi[NG], ci = 0.f;
#pragma unroll
    for (int i = 0; i < NG; ++i) gi[i] = 0.f;
    if (len > 0) g.input(rows, gi, ci);
    for (int t = 0; t < len; ++t) {
      float gn[NG], cn = 0.f;
#pragma unroll
      for (int i = 0; i < NG; ++i) gn[i] = 0.f;
      if (t + 1 < len) g.input(rows + (t + 1) * RW, gn, cn);
      float u, c;
      g.step(gi, ci, h, half, u, c);
      h = fmaf(u, h - c, c);  // u*h + (1-u)*c
      if (p < NH) rows[t * RW + j] = h;
      if constexpr (SAVE) {
        if (p < NH) hs_out[(b * T + t) * NH + j] = h;
      }
#pragma unroll
      for (int i = 0; i < NG; ++i) gi[i] = gn[i];
      ci = cn;
    }
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
          const f32x4 v = *reinterpret_cast<const f32x4*>(rows + t * RW + 4 * c4);
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
    g.load(w.Vg, w.vg, w.Vc, w.vc, p);
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
        g.input(rows + (t + 1) * RW, gn, cn);
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
      if constexpr (SAVE) {
        if (p < NH) ss_out[(b * T + t) * NH + j] = st;
      }
#pragma unroll
      for (int i = 0; i < NG; ++i) gi[i] = gn[i];
      ci = cn;
      a = an;
    }
    if (live && p < NH) out[b * ld_out + j] = st;
  }
  if constexpr (SAVE) {
    if (live)
      for (int e = len * NH + p; e < T * NH; e += 16) {
        hs_out[b * T * NH + e] = 0.f;
        ss_out[b * T * NH + e] = 0.f;
      }
  }
}

// Floats of LDS per sample: the rows, the scores and A . e_target, padded so that the four
// samples of a wave start 16 banks apart (their broadcast float4 row reads never collide).
static int dien_sample_stride(int T, int H, int NH) {
  const int rw = H > NH ? H : NH;
  const int base = T * rw + ((T + 3) & ~3) + 16;
  return base + ((16 - base % 64) + 64) % 64;
}

}  // namespace rk

using namespace rk;

static int launch_dien(const float* query, int64_t ld_query, const float* key_table, int64_t key_rows,
                       int64_t ld_key, const int64_t* seq, int64_t ld_seq, int64_t ld_kb, int32_t T,
                       const int64_t* seq_len, int64_t batch, int32_t H, int32_t nh, int32_t cell_type,
                       const DienWeights& w, float* out, int64_t ld_out, float* att_out, int64_t ld_att,
                       void* stream, const char* who, bool save = false, float* hs_out = nullptr,
                       float* ss_out = nullptr) {
  if (!query || !key_table || !seq_len || !w.Wg || !w.bg || !w.Wc || !w.bc || !w.A || !w.Vg || !w.vg || !w.Vc ||
      !w.vc || !out || (save && (!hs_out || !ss_out || !att_out)))
    return fail(RK_ERR_INVALID, "%s: null pointer", who);
  if (T <= 0 || batch < 0 || H <= 0 || nh <= 0 || ld_query < H || ld_out < nh || ld_key < H || (att_out && ld_att < T))
    return fail(RK_ERR_INVALID, "%s: bad shape T=%d H=%d nh=%d", who, T, H, nh);
  if (cell_type != 0 && cell_type != 1)
    return fail(RK_ERR_INVALID, "%s: cell_type %d is neither 0 (AGRU) nor 1 (AUGRU)", who, cell_type);
  if ((H != 8 && H != 16 && H != 32) || (nh != 8 && nh != 16) || T > 256)
    return fail(RK_ERR_UNSUPPORTED, "%s: H=%d nh=%d T=%d outside the envelope H in {8,16,32}, nh in {8,16}, T <= 256",
                who, H, nh, T);
  if (ld_key % 4 != 0 || ld_kb % 4 != 0 || ((uintptr_t)key_table & 15u))
    return fail(RK_ERR_UNSUPPORTED, "%s: history rows must be 16-B aligned", who);
  if (batch == 0) return RK_OK;
  const int stride = dien_sample_stride(T, H, nh);
  const size_t shm = (size_t)kDienSamples * stride * sizeof(float);
  const unsigned blocks = (unsigned)((batch + kDienSamples - 1) / kDienSamples);
  hipStream_t st = (hipStream_t)stream;
  uint32_t* fl = device_flags();
#define RK_DIEN_LAUNCH(HH, NN, SV)                                                                            \
  if (shm > 64 * 1024) raise_lds_limit((const void*)dien_interest_kernel<HH, NN, SV>, (int)shm);              \
  dien_interest_kernel<HH, NN, SV><<<blocks, 64, shm, st>>>(query, ld_query, key_table, key_rows, ld_key, seq, \
                                                            ld_seq, ld_kb, T, seq_len, batch, w, cell_type,   \
                                                            stride, out, ld_out, att_out, ld_att, fl, hs_out, \
                                                            ss_out);
#define RK_DIEN_CASE(HH, NN)                                                                                  \
  if (H == HH && nh == NN) {                                                                                  \
    if (save) {                                                                                               \
      RK_DIEN_LAUNCH(HH, NN, true)                                                                            \
    } else {                                                                                                  \
      RK_DIEN_LAUNCH(HH, NN, false)                                                                           \
    }                                                                                                         \
  }
  RK_DIEN_CASE(8, 8)
  RK_DIEN_CASE(16, 8)
  RK_DIEN_CASE(32, 8)
  RK_DIEN_CASE(8, 16)
  RK_DIEN_CASE(16, 16)
  RK_DIEN_CASE(32, 16)
#undef RK_DIEN_CASE
#undef RK_DIEN_LAUNCH
  return check_launch(who);
}

RK_API int rk_dien_interest(const float* query, int64_t ld_query, const float* key_table, int64_t key_rows,
                            int64_t ld_key, const int64_t* seq, int64_t ld_seq, int32_t T, const int64_t* seq_len,
                            int64_t batch, int32_t H, int32_t nh, int32_t cell_type, const float* Wg,
                            const float* bg, const float* Wc, const float* bc, const float* A, const float* Vg,
                            const float* vg, const float* Vc, const float* vc, float* out, int64_t ld_out,
                            float* att_out, int64_t ld_att, void* stream) {
  if (!seq) return fail(RK_ERR_INVALID, "rk_dien_interest: null pointer");
  if (key_rows <= 0 || ld_seq < T) return fail(RK_ERR_INVALID, "rk_dien_interest: bad shape T=%d", T);
  const DienWeights w{Wg, bg, Wc, bc, A, Vg, vg, Vc, vc};
  return launch_dien(query, ld_query, key_table, key_rows, ld_key, seq, ld_seq, 0, T, seq_len, batch, H, nh,
                     cell_type, w, out, ld_out, att_out, ld_att, stream, "rk_dien_interest");
}

RK_API int rk_dien_interest_dense(const float* query, int64_t ld_query, const float* keys, int64_t ld_keys_b,
                                  int64_t ld_keys_t, int32_t T, const int64_t* keys_length, int64_t batch,
                                  int32_t H, int32_t nh, int32_t cell_type, const float* Wg, const float* bg,
                                  const float* Wc, const float* bc, const float* A, const float* Vg,
                                  const float* vg, const float* Vc, const float* vc, float* out, int64_t ld_out,
                                  float* att_out, int64_t ld_att, void* stream) {
  if (T > 0 && ld_keys_b < (int64_t)T * ld_keys_t && batch > 1)
    return fail(RK_ERR_INVALID, "rk_dien_interest_dense: bad shape T=%d", T);
  const DienWeights w{Wg, bg, Wc, bc, A, Vg, vg, Vc, vc};
  return launch_dien(query, ld_query, keys, 0, ld_keys_t, nullptr, 0, ld_keys_b, T, keys_length, batch, H, nh,
                     cell_type, w, out, ld_out, att_out, ld_att, stream, "rk_dien_interest_dense");
}

RK_API int rk_dien_interest_train(const float* query, int64_t ld_query, const float* key_table, int64_t key_rows,
                                  int64_t ld_key, const int64_t* seq, int64_t ld_seq, int32_t T,
                                  const int64_t* seq_len, int64_t batch, int32_t H, int32_t nh, int32_t cell_type,
                                  const float* Wg, const float* bg, const float* Wc, const float* bc, const float* A,
                                  const float* Vg, const float* vg, const float* Vc, const float* vc, float* out,
                                  int64_t ld_out, float* att_out, int64_t ld_att, float* hs, float* ss,
                                  void* stream) {
  if (!seq) return fail(RK_ERR_INVALID, "rk_dien_interest_train: null pointer");
  if (key_rows <= 0 || ld_seq < T) return fail(RK_ERR_INVALID, "rk_dien_interest_train: bad shape T=%d", T);
  const DienWeights w{Wg, bg, Wc, bc, A, Vg, vg, Vc, vc};
  return launch_dien(query, ld_query, key_table, key_rows, ld_key, seq, ld_seq, 0, T, seq_len, batch, H, nh,
                     cell_type, w, out, ld_out, att_out, ld_att, stream, "rk_dien_interest_train", true, hs, ss);
}

RK_API int rk_dien_interest_train_dense(const float* query, int64_t ld_query, const float* keys, int64_t ld_keys_b,
                                        int64_t ld_keys_t, int32_t T, const int64_t* keys_length, int64_t batch,
                                        int32_t H, int32_t nh, int32_t cell_type, const float* Wg, const float* bg,
                                        const float* Wc, const float* bc, const float* A, const float* Vg,
                                        const float* vg, const float* Vc, const float* vc, float* out,
                                        int64_t ld_out, float* att_out, int64_t ld_att, float* hs, float* ss,
                                        void* stream) {
  if (T > 0 && ld_keys_b < (int64_t)T * ld_keys_t && batch > 1)
    return fail(RK_ERR_INVALID, "rk_dien_interest_train_dense: bad shape T=%d", T);
  const DienWeights w{Wg, bg, Wc, bc, A, Vg, vg, Vc, vc};
  return launch_dien(query, ld_query, keys, 0, ld_keys_t, nullptr, 0, ld_keys_b, T, keys_length, batch, H, nh,
                     cell_type, w, out, ld_out, att_out, ld_att, stream, "rk_dien_interest_train_dense", true, hs,
                     ss);
}
