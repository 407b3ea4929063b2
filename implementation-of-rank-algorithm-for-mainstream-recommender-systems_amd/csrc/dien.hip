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
// dense form run the same code after the gather.  The phases themselves are in dien_cell.h.
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
  extern __shared__ __attribute__((aligned(16))) float dien_sm[];
  const int lane = threadIdx.x, p = lane & 15, s = lane >> 4;
  const int64_t b = (int64_t)blockIdx.x * kDienSamples + s;
  const bool live = b < batch;
  float* rows = dien_sm + (size_t)s * sample_stride;  // [T][RW]
  float* att = rows + T * RW;                          // [T]: scores, then attention weights
  float* wea = att + ((T + 3) & ~3);                   // [NH]: A . e_target
  const int len = live ? dien_len(seq_len, b, T) : 0;

  dien_gather_rows<H, RW>(key_table, key_rows, ld_key, seq, ld_seq, ld_kb, b, len, p, flags, rows);
  dien_project_query<H, NH>(w.A, query, ld_query, b, live, p, wea);
  __syncthreads();
  dien_extract_pass<H, NH, RW, true, SAVE>(w.Wg, w.bg, w.Wc, w.bc, rows, len, p, hs_out, b, T);
  __syncthreads();
  dien_attention<NH, RW>(rows, wea, att, T, len, p, att_out, ld_att, b, live);
  __syncthreads();
  dien_evolve_pass<NH, RW, SAVE>(w.Vg, w.vg, w.Vc, w.vc, rows, att, len, p, cell_type, ss_out, b, T, out, ld_out,
                                 live);
  if constexpr (SAVE) {
    if (live)
      for (int e = len * NH + p; e < T * NH; e += 16) {
        hs_out[b * T * NH + e] = 0.f;
        ss_out[b * T * NH + e] = 0.f;
      }
  }
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
  if (int rc = dien_check_cell(who, cell_type)) return rc;
  if (int rc = dien_check_envelope(who, H, nh, T)) return rc;
  if (int rc = dien_check_history_rows(who, key_table, ld_key, ld_kb)) return rc;
  if (batch == 0) return RK_OK;
  // floats of LDS per sample: the rows, the scores and A . e_target
  const int stride = dien_padded_stride(T * (H > nh ? H : nh) + ((T + 3) & ~3) + 16);
  const size_t shm = (size_t)kDienSamples * stride * sizeof(float);
  const unsigned blocks = (unsigned)((batch + kDienSamples - 1) / kDienSamples);
  dien_launch(
      H, nh,
      [save](auto s) { return save ? dien_interest_kernel<s.H, s.NH, true> : dien_interest_kernel<s.H, s.NH, false>; },
      blocks, shm, (hipStream_t)stream, query, ld_query, key_table, key_rows, ld_key, seq, ld_seq, ld_kb, T, seq_len,
      batch, w, cell_type, stride, out, ld_out, att_out, ld_att, device_flags(), hs_out, ss_out);
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
