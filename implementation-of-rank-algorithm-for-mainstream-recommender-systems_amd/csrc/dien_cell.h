// DIEN kernels (dien.hip, dien_train.hip): the GRU-shaped cell as one DPP row of 16 lanes sees it, and
// the helpers both the forward and the backward chain use.
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

}  // namespace rk
