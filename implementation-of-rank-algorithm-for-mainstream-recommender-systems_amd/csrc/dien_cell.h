// DIEN kernels (dien.hip, dien_requests.hip, dien_train.hip): the GRU-shaped cell as one DPP row of 16
// lanes sees it, the phases of the forward, written once for the fused kernel (dien.hip) and its two
// halves (dien_requests.hip), and the host checks, LDS padding and dispatch that every launch shares.
#pragma once
#include "common.h"

namespace rk {

constexpr int kDienSamples = 4;  // samples per wave (= per workgroup)

struct DienWeights {
  const float *Wg, *bg, *Wc, *bc, *A, *Vg, *vg, *Vc, *vc;
};

template <int K>
__device__ __forceinline__ float row_ror(float v) {
  if constexpr (K == 0)
    return v;
  else
    // row_ror:K; every lane of a row is a valid source, so bound_ctrl changes nothing but lets the
    // compiler fold the move into the consuming v_fmac_f32
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x120 + K, 0xF, 0xF, true));
}
// The lane (of the 16 of a row) whose value row_ror<K> delivers to lane p, asked of the hardware.
template <int K>
__device__ __forceinline__ int row_ror_source(int p) {
  if constexpr (K == 0)
    return p;
  else
    return __builtin_amdgcn_update_dpp(0, p, 0x120 + K, 0xF, 0xF, false);
}

// tanh on the transcendental unit: 2 * sigmoid(2x) - 1; absolute error ~1e-7, saturates to +-1.
__device__ __forceinline__ float tanh_fast(float x) {
  return fmaf(2.0f, __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * -2.88539008177792681f)), -1.0f);
}

// One GRU-shaped cell (XW inputs, NH units) as lane p of a sample's row sees it.
template <int XW, int NH>
struct DienCell {
  static constexpr int NG = NH / 8;  // gate rows per lane: nh 8 -> row p; nh 16 -> rows p and p + 16
  static constexpr int LD = XW + NH;
  float gx[NG][XW], cx[XW];  // input halves of this lane's gate rows / candidate row
  float gh[NG][NH], ch[NH];  // state halves, in rotation order
  float gb[NG], cb;

  template <int K>
  __device__ __forceinline__ void load_rot(const float* Wg, const float* Wc, int p) {
    const int unit = row_ror_source<K>(p) % NH;  // the unit whose state rotation K brings here
#pragma unroll
    for (int i = 0; i < NG; ++i) gh[i][K] = Wg[(p + 16 * i) * LD + XW + unit];
    ch[K] = Wc[(p % NH) * LD + XW + unit];
    if constexpr (K + 1 < NH) load_rot<K + 1>(Wg, Wc, p);
  }

  __device__ __forceinline__ void load(const float* Wg, const float* bg, const float* Wc, const float* bc, int p) {
#pragma unroll
    for (int i = 0; i < NG; ++i) {
#pragma unroll
      for (int x = 0; x < XW; ++x) gx[i][x] = Wg[(p + 16 * i) * LD + x];
      gb[i] = bg[p + 16 * i];
    }
#pragma unroll
    for (int x = 0; x < XW; ++x) cx[x] = Wc[(p % NH) * LD + x];
    cb = bc[p % NH];
    load_rot<0>(Wg, Wc, p);
  }

  // Input halves (+ bias) of one step from the LDS row x (16-B aligned, XW floats).
  __device__ __forceinline__ void input(const float* x, float (&gi)[NG], float& ci) const {
#pragma unroll
    for (int i = 0; i < NG; ++i) gi[i] = gb[i];
    ci = cb;
#pragma unroll
    for (int c4 = 0; c4 < XW / 4; ++c4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(x + 4 * c4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int i = 0; i < NG; ++i) gi[i] = fmaf(gx[i][4 * c4 + e], v[e], gi[i]);
        ci = fmaf(cx[4 * c4 + e], v[e], ci);
      }
    }
  }

  template <int K>
  __device__ __forceinline__ void gate_dot(float (&acc)[NG], float h) const {
    const float hk = row_ror<K>(h);
#pragma unroll
    for (int i = 0; i < NG; ++i) acc[i] = fmaf(hk, gh[i][K], acc[i]);
    if constexpr (K + 1 < NH) gate_dot<K + 1>(acc, h);
  }
  template <int K>
  __device__ __forceinline__ void cand_dot(float& acc, float rh) const {
    acc = fmaf(row_ror<K>(rh), ch[K], acc);
    if constexpr (K + 1 < NH) cand_dot<K + 1>(acc, rh);
  }

  // Update gate u and candidate c of this lane's unit from the input halves and the state h.
  __device__ __forceinline__ void step(const float (&gi)[NG], float ci, float h, int half, float& u,
                                       float& c) const {
    float r;
    gates(gi, ci, h, half, r, u, c);
  }

  // The same with the reset gate r handed out too (the backward recomputes all three).
  __device__ __forceinline__ void gates(const float (&gi)[NG], float ci, float h, int half, float& r, float& u,
                                        float& c) const {
    float acc[NG];
#pragma unroll
    for (int i = 0; i < NG; ++i) acc[i] = gi[i];
    gate_dot<0>(acc, h);
    if constexpr (NG == 1) {  // lanes 0-7 hold r, lanes 8-15 hold u of the same units
      const float g = sigmoid_fast(acc[0]);
      const float o = row_ror<8>(g);
      r = half ? o : g;
      u = half ? g : o;
    } else {
      r = sigmoid_fast(acc[0]);
      u = sigmoid_fast(acc[NG - 1]);
    }
    float ac = ci;
    cand_dot<0>(ac, r * h);
    c = tanh_fast(ac);
  }
};

// ---- The phases of the forward.  dien_interest_kernel<., ., false / true>, dien_extract_kernel and
// dien_evolve_kernel are compositions of these, which is why their results are bit-equal: p is the
// lane within the sample's row of 16, b the sample, RW the width in floats of an LDS row.  The kernels
// keep their LDS carve-up, the barriers between the phases and the zero-fill of what they store.

// A sample's history length, clamped to [0, T].
__device__ __forceinline__ int dien_len(const int64_t* __restrict__ seq_len, int64_t b, int T) {
  const int64_t l = seq_len[b];
  return l < 0 ? 0 : (l > T ? T : (int)l);
}

// The sample's len history rows into LDS: lane p resolves position t0 + p (an id of the table, or the
// dense row when seq is null), then the 16 lanes copy the 16 rows as float4 chunks (control flow is
// uniform over a sample's row).  An out-of-range id reads zeros and raises the flag.
template <int H, int RW>
__device__ __forceinline__ void dien_gather_rows(const float* __restrict__ key_table, int64_t key_rows,
                                                 int64_t ld_key, const int64_t* __restrict__ seq, int64_t ld_seq,
                                                 int64_t ld_kb, int64_t b, int len, int p, uint32_t* flags,
                                                 float* rows) {
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
}

// A . e_target into wea [NH], one unit per lane (zeros for a sample past the batch).
template <int H, int NH>
__device__ __forceinline__ void dien_project_query(const float* A, const float* query, int64_t ld_query, int64_t b,
                                                   bool live, int p, float* wea) {
  const int j = p % NH;
  float a = 0.f;
  if (live) {
    const float* q = query + b * ld_query;
#pragma unroll
    for (int i = 0; i < H; ++i) a = fmaf(A[j * H + i], q[i], a);
  }
  if (p < NH) wea[j] = a;
}

// Pass 1, the interest extractor over the x_t in rows, the input halves one step ahead of the state.
// h_t goes over row t (TO_LDS) and / or to hs_out [., T, NH] (TO_GLOBAL).
template <int H, int NH, int RW, bool TO_LDS, bool TO_GLOBAL>
__device__ __forceinline__ void dien_extract_pass(const float* Wg, const float* bg, const float* Wc, const float* bc,
                                                  float* rows, int len, int p, float* __restrict__ hs_out, int64_t b,
                                                  int T) {
  constexpr int NG = NH / 8;
  const int j = p % NH, half = p >> 3;
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
    if (t + 1 < len) g.input(rows + (t + 1) * RW, gn, cn);
    float u, c;
    g.step(gi, ci, h, half, u, c);
    h = fmaf(u, h - c, c);  // u*h + (1-u)*c
    if constexpr (TO_LDS) {
      if (p < NH) rows[t * RW + j] = h;
    }
    if constexpr (TO_GLOBAL) {
      if (p < NH) hs_out[(b * T + t) * NH + j] = h;
    }
#pragma unroll
    for (int i = 0; i < NG; ++i) gi[i] = gn[i];
    ci = cn;
  }
}

// Scores h_t . wea for t < len, the pad past it, and the softmax over all T positions into att [T]
// (and att_out, if given); lane p takes t = p, p + 16, ...
template <int NH, int RW>
__device__ __forceinline__ void dien_attention(const float* rows, const float* wea, float* att, int T, int len, int p,
                                               float* __restrict__ att_out, int64_t ld_att, int64_t b, bool live) {
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

// Pass 2, the interest evolution (cell_type 0 AGRU, 1 AUGRU) over h_t in rows and a_t in att, t < len,
// both read one step ahead; SAVE: s_t also goes to ss_out [., T, NH].  The final state goes to out[b] from
// in here, as it did before the phases were lifted out: handed back for the kernel to store, several
// instantiations came out with one more s_waitcnt inside the loop (the wait for the last weight).
// dien_evolve_kernel restates this pass (dien_requests.hip says why).
template <int NH, int RW, bool SAVE>
__device__ __forceinline__ void dien_evolve_pass(const float* Vg, const float* vg, const float* Vc, const float* vc,
                                                 const float* rows, const float* att, int len, int p, int cell_type,
                                                 float* __restrict__ ss_out, int64_t b, int T, float* out,
                                                 int64_t ld_out, bool live) {
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

// ---- Host side: what the launches of the four files check and compute alike.

// A sample's LDS stride for `floats` floats of its own: padded so that the four samples of a wave
// start 16 banks apart (their broadcast float4 row reads never collide).
inline int dien_padded_stride(int floats) { return floats + ((16 - floats % 64) + 64) % 64; }

inline int dien_check_cell(const char* who, int cell_type) {
  if (cell_type != 0 && cell_type != 1)
    return fail(RK_ERR_INVALID, "%s: cell_type %d is neither 0 (AGRU) nor 1 (AUGRU)", who, cell_type);
  return RK_OK;
}

inline int dien_check_envelope(const char* who, int H, int nh, int T) {
  if ((H != 8 && H != 16 && H != 32) || (nh != 8 && nh != 16) || T > 256)
    return fail(RK_ERR_UNSUPPORTED, "%s: H=%d nh=%d T=%d outside the envelope H in {8,16,32}, nh in {8,16}, T <= 256",
                who, H, nh, T);
  return RK_OK;
}

// The gather copies history rows as float4.
inline int dien_check_history_rows(const char* who, const float* key_table, int64_t ld_key, int64_t ld_kb) {
  if (ld_key % 4 != 0 || ld_kb % 4 != 0 || ((uintptr_t)key_table & 15u))
    return fail(RK_ERR_UNSUPPORTED, "%s: history rows must be 16-B aligned", who);
  return RK_OK;
}

template <int HH, int NN>
struct DienShape {
  static constexpr int H = HH, NH = NN;
};

// Launches pick(DienShape<H, nh>{}), the caller's kernel instantiated for the envelope's (H, nh) pair,
// over `blocks` workgroups of one wave with `shm` bytes of LDS (raised past the 64 KB default first).
template <class Pick, class... Args>
inline void dien_launch(int H, int nh, Pick pick, unsigned blocks, size_t shm, hipStream_t st, Args... args) {
  auto go = [&](auto kernel) {
    if (shm > 64 * 1024) raise_lds_limit((const void*)kernel, (int)shm);
    kernel<<<blocks, 64, shm, st>>>(args...);
  };
  if (H == 8 && nh == 8) go(pick(DienShape<8, 8>{}));
  if (H == 16 && nh == 8) go(pick(DienShape<16, 8>{}));
  if (H == 32 && nh == 8) go(pick(DienShape<32, 8>{}));
  if (H == 8 && nh == 16) go(pick(DienShape<8, 16>{}));
  if (H == 16 && nh == 16) go(pick(DienShape<16, 16>{}));
  if (H == 32 && nh == 16) go(pick(DienShape<32, 16>{}));
}

}  // namespace rk
