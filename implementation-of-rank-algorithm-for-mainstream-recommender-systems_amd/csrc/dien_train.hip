// DIEN interest extractor + interest evolution, backward (training; the forward that keeps hs / ss /
// att is dien_interest_kernel<H, NH, true> in dien.hip).  FP32, one chain launch plus GEMMs.
//
// Backprop through time of tests/dien_ref.py::interest, t = len-1 ... 0, given d_out = dL/d(state):
//   evolution step t (gates r, u, c from (h_t, s_{t-1}), a = att_t):
//     AGRU:   da_t = sum_j ds (c - s_{t-1});  dc = a ds;  direct = (1-a) ds;  du = 0
//     AUGRU:  u' = (1-a) u;  du' = ds (s_{t-1} - c);  da_t = -sum_j du' u;  du = (1-a) du'
//             dc = (1-u') ds;  direct = u' ds
//     dpc = dc (1-c^2);  d(r s) = Vc[:, nh:]^T dpc;  dpr = d(r s) s_{t-1} r (1-r);  dpu = du u (1-u)
//     ds_{t-1} = direct + d(r s) r + Vg[:, nh:]^T [dpr|dpu];  dh_t = Vg[:, :nh]^T [dpr|dpu] + Vc[:, :nh]^T dpc
//   attention:  dscore_t = a_t (da_t - sum_tau a_tau da_tau);  dh_t += dscore_t (A q)
//               d(A q) = sum_t dscore_t h_t;  dq = A^T d(A q)
//   extractor step t (gates from (x_t, h_{t-1})):  du = dh (h_{t-1} - c);  dc = dh (1-u);  direct = u dh,
//     then as above with Wg / Wc;  dx_t = Wg[:, :H]^T [dpr|dpu] + Wc[:, :H]^T dpc
//   rk_dien_interest_backward_aux: dh_t also takes d_hs[b, t] (t < len), the gradient the auxiliary loss
//     (dien_aux.hip) sends into the extractor states, and dkeys may be added to what that loss wrote
//
// Work split as in the forward: one DPP row (16 lanes) per sample, lane p holds unit p % nh.  The
// gates of step t depend only on saved states, so they are recomputed with the forward's DienCell
// one step ahead of the ds / dh they meet; the dependent chain is the two transposed state mat-vecs,
// run as row_ror rotations over transposed weights held in registers in rotation order (nh = 8:
// lanes 0-7 carry dpr and lanes 8-15 dpu, each half sums 8 of the 16 gate rows, one row_ror:8 adds
// the halves).  dh_t, da_t / dscore_t, a_t and the key row offsets live in LDS; x_t, h_t, s_t stream
// from global memory.
//
// Weight gradients: the kernel writes, per (b, t), the pre-activation gradients G = [dpr|dpu|dpc]
// and the operand rows O = [x_t | h_{t-1} | r*h_{t-1}] of both cells (rows t >= len zero in both), and
// d(A q) with a copy of q; the nine dW / db are three rk_gemm_wgrad products over those rows (G^T O per
// cell, unpacked into its blocks, and dA; fixed-order partial sums, no float atomics), and dkeys = G1 . [Wg[:, :H]; Wc[:, :H]] is two rk_gemm calls, so the
// chain kernel's registers stay with the chain.  Everything is deterministic.
#include "dien_cell.h"

namespace rk {

// Transposed halves of one cell's weights as lane p (destination column k = p % NH of the state
// half, or of the input half when that is NH wide too) needs them under row_ror rotations.
template <int XW, int NH, bool INPUT>
struct DienCellT {
  static constexpr int NG = NH / 8;
  static constexpr int LD = XW + NH;
  float gh[NG][NH], ch[NH];  // state half:  Wg[row, XW + k], Wc[unit, XW + k]
  float gx[NG][NH], cx[NH];  // input half (INPUT, XW == NH):  Wg[row, k], Wc[unit, k]

  template <int K>
  __device__ __forceinline__ void load_rot(const float* Wg, const float* Wc, int p) {
    const int q = row_ror_source<K>(p);  // the lane whose gradients rotation K brings here
    const int k = p % NH;
#pragma unroll
    for (int i = 0; i < NG; ++i) {
      gh[i][K] = Wg[(q + 16 * i) * LD + XW + k];
      if constexpr (INPUT) gx[i][K] = Wg[(q + 16 * i) * LD + k];
    }
    ch[K] = Wc[(q % NH) * LD + XW + k];
    if constexpr (INPUT) cx[K] = Wc[(q % NH) * LD + k];
    if constexpr (K + 1 < NH) load_rot<K + 1>(Wg, Wc, p);
  }
  __device__ __forceinline__ void load(const float* Wg, const float* Wc, int p) { load_rot<0>(Wg, Wc, p); }

  template <int K>
  __device__ __forceinline__ void cand_t(float& acc, float& accx, float dpc) const {
    const float v = row_ror<K>(dpc);
    acc = fmaf(v, ch[K], acc);
    if constexpr (INPUT) accx = fmaf(v, cx[K], accx);
    if constexpr (K + 1 < NH) cand_t<K + 1>(acc, accx, dpc);
  }
  // g: NG == 1 this lane's gate-row gradient (dpr in lanes 0-7, dpu in 8-15); NG == 2 {dpr, dpu}
  template <int K>
  __device__ __forceinline__ void gate_t(float& acc, float& accx, const float (&g)[NG]) const {
#pragma unroll
    for (int i = 0; i < NG; ++i) {
      const float v = row_ror<K>(g[i]);
      acc = fmaf(v, gh[i][K], acc);
      if constexpr (INPUT) accx = fmaf(v, gx[i][K], accx);
    }
    if constexpr (K + 1 < NH) gate_t<K + 1>(acc, accx, g);
  }

  // d(r*state) = Wc[:, XW:]^T dpc; accx (+)= Wc[:, :XW]^T dpc
  __device__ __forceinline__ float cand(float dpc, float& accx) const {
    float acc = 0.f;
    cand_t<0>(acc, accx, dpc);
    return acc;
  }
  // Wg[:, XW:]^T [dpr|dpu]; accx (+)= Wg[:, :XW]^T [dpr|dpu]
  __device__ __forceinline__ float gate(float dpr, float dpu, int half, float& accx) const {
    float acc = 0.f, ax = 0.f, g[NG];
    if constexpr (NG == 1) {
      g[0] = half ? dpu : dpr;
    } else {
      g[0] = dpr;
      g[NG - 1] = dpu;
    }
    gate_t<0>(acc, ax, g);
    if constexpr (NG == 1) {  // each half summed 8 of the 16 gate rows
      acc += row_ror<8>(acc);
      if constexpr (INPUT) ax += row_ror<8>(ax);
    }
    accx += ax;
    return acc;
  }
};

struct DienGrads {
  float *dquery, *g1, *o1, *g2, *o2, *dwea, *qc;
  int64_t* seq_masked;  // [batch, T] or null: the ids with 0 at t >= len, for the embedding scatter
};

template <int H, int NH>
__global__ __launch_bounds__(64) void dien_interest_backward_kernel(
    const float* query, int64_t ld_query, const float* __restrict__ key_table, int64_t key_rows, int64_t ld_key,
    const int64_t* __restrict__ seq, int64_t ld_seq, int64_t ld_kb, int T, const int64_t* __restrict__ seq_len,
    int64_t batch, DienWeights w, int cell_type, int sample_stride, const float* __restrict__ hs,
    const float* __restrict__ ss, const float* __restrict__ att_in, int64_t ld_att, const float* d_out,
    int64_t ld_dout, int64_t ld_dquery, int accumulate, DienGrads gr, const float* __restrict__ d_hs) {
  constexpr int NG = NH / 8;
  constexpr int LO1 = H + 2 * NH, LG = 3 * NH;  // row widths of O1 and of G1 / G2 / O2
  extern __shared__ __attribute__((aligned(16))) float dien_bsm[];
  const int lane = threadIdx.x, p = lane & 15, s = lane >> 4, j = p % NH, half = p >> 3;
  const int64_t b = (int64_t)blockIdx.x * kDienSamples + s;
  const bool live = b < batch;
  float* zero_row = dien_bsm;  // [32] zeros: the key row of an out-of-range id (as the forward reads it)
  float* sm = dien_bsm + 32 + (size_t)s * sample_stride;
  const int T4 = (T + 3) & ~3;
  float* dh = sm;                 // [T][NH]: dL/dh_t from the evolution's input half
  float* da = dh + T * NH;        // [T]: da_t, then dscore_t
  float* att = da + T4;           // [T]
  float* wea = att + T4;          // [NH]: A . e_target
  float* dwl = wea + 16;          // [NH]: d(A . e_target)
  long long* offs = reinterpret_cast<long long*>(dwl + 16);  // [T]: element offset of key row t, -1: zero row
  const int len = live ? dien_len(seq_len, b, T) : 0;
  if (lane < 32) zero_row[lane] = 0.f;
  for (int t = p; t < len; t += 16) {
    long long off = -1;
    if (seq) {
      const int64_t r = seq[b * ld_seq + t];
      if (r >= 0 && r < key_rows) off = r * ld_key;
    } else {
      off = b * ld_kb + (int64_t)t * ld_key;
    }
    offs[t] = off;
    att[t] = att_in[b * ld_att + t];
  }
  {  // dien_project_query, restated: the call moves <8,16> from 32 to 30 AGPRs, and these figures are pinned
    float a = 0.f;
    if (live) {
      const float* q = query + b * ld_query;
#pragma unroll
      for (int i = 0; i < H; ++i) a = fmaf(w.A[j * H + i], q[i], a);
    }
    if (p < NH) wea[j] = a;
  }
  // rows t >= len of the gradient and operand buffers are zero (their products must be exact zeros)
  if (live) {
    const int64_t r0 = b * T;
    for (int e = len * LG + p; e < T * LG; e += 16) {
      gr.g1[r0 * LG + e] = 0.f;
      gr.g2[r0 * LG + e] = 0.f;
      gr.o2[r0 * LG + e] = 0.f;
    }
    for (int e = len * LO1 + p; e < T * LO1; e += 16) gr.o1[r0 * LO1 + e] = 0.f;
    if (seq && gr.seq_masked)
      for (int t = p; t < T; t += 16) gr.seq_masked[r0 + t] = t < len ? seq[b * ld_seq + t] : 0;
  }
  __syncthreads();
  const float* hsb = hs + (live ? b : 0) * T * NH;
  const float* ssb = ss + (live ? b : 0) * T * NH;
  // an extra dL/dh_t from outside the recurrence (the auxiliary loss), or null; rows t < len only
  const float* dxb = d_hs ? d_hs + (live ? b : 0) * T * NH : nullptr;

  // ---- pass 1: interest evolution backward, t = len-1 ... 0
  {
    DienCell<NH, NH> g;
    g.load(w.Vg, w.vg, w.Vc, w.vc, p);
    DienCellT<NH, NH, true> gt;
    gt.load(w.Vg, w.Vc, p);
    float ds = len > 0 ? d_out[b * ld_dout + j] : 0.f;
    float r = 0.f, u = 0.f, c = 0.f, sp = 0.f, ht = 0.f, a = 0.f;
    if (len > 0) {
      const int t = len - 1;
      float gi[NG], ci;
      g.input(hsb + t * NH, gi, ci);
      sp = t > 0 ? ssb[(t - 1) * NH + j] : 0.f;
      ht = hsb[t * NH + j];
      a = att[t];
      g.gates(gi, ci, sp, half, r, u, c);
    }
    for (int t = len - 1; t >= 0; --t) {
      float rn = 0.f, un = 0.f, cn = 0.f, spn = 0.f, htn = 0.f, an = 0.f;
      if (t > 0) {  // the gates of step t-1: saved states only
        float gi[NG], ci;
        g.input(hsb + (t - 1) * NH, gi, ci);
        spn = t > 1 ? ssb[(t - 2) * NH + j] : 0.f;
        htn = hsb[(t - 1) * NH + j];
        an = att[t - 1];
        g.gates(gi, ci, spn, half, rn, un, cn);
      }
      float dat, dc, direct, dpu;
      if (cell_type == 0) {
        dat = ds * (c - sp);
        dc = a * ds;
        direct = ds - dc;
        dpu = 0.f;
      } else {
        const float u2 = fmaf(-a, u, u);
        const float du2 = ds * (sp - c);
        dat = -du2 * u;
        dc = fmaf(-u2, ds, ds);
        direct = u2 * ds;
        dpu = fmaf(-a, du2, du2) * u * (1.0f - u);
      }
      const float dpc = dc * fmaf(-c, c, 1.0f);
      float dhx = 0.f;
      const float drs = gt.cand(dpc, dhx);
      const float dpr = drs * sp * r * (1.0f - r);
      const float back = gt.gate(dpr, dpu, half, dhx);
      ds = direct + fmaf(drs, r, back);
      // off the chain: da_t, dL/dh_t, and this step's rows of G2 / O2
      const float dsum = row16_sum(p < NH ? dat : 0.f);
      if (p == 0) da[t] = dsum;
      if (p < NH) {
        dh[t * NH + j] = dhx;
        float* g2 = gr.g2 + (b * T + t) * LG;
        float* o2 = gr.o2 + (b * T + t) * LG;
        g2[j] = dpr;
        g2[NH + j] = dpu;
        g2[2 * NH + j] = dpc;
        o2[j] = ht;
        o2[NH + j] = sp;
        o2[2 * NH + j] = r * sp;
      }
      r = rn, u = un, c = cn, sp = spn, ht = htn, a = an;
    }
  }
  __syncthreads();

  // ---- attention backward: dscore_t = a_t (da_t - sum a da), d(A q) = sum_t dscore_t h_t, dq = A^T d(A q)
  {
    float dot = 0.f;
    for (int t = p; t < len; t += 16) dot = fmaf(att[t], da[t], dot);
    dot = row16_sum(dot);
    for (int t = p; t < len; t += 16) da[t] = att[t] * (da[t] - dot);
    __syncthreads();
    float dw = 0.f;
    for (int t = 0; t < len; ++t) dw = fmaf(da[t], hsb[t * NH + j], dw);
    if (p < NH) dwl[j] = dw;
    __syncthreads();
    if (live) {
      if (p < NH) gr.dwea[b * NH + j] = dw;
      const float* q = query + b * ld_query;
      for (int i = p; i < H; i += 16) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < NH; ++k) acc = fmaf(w.A[k * H + i], dwl[k], acc);
        gr.qc[b * H + i] = q[i];
        float* d = gr.dquery + b * ld_dquery + i;
        *d = accumulate ? *d + acc : acc;
      }
    }
  }

  // ---- pass 2: interest extractor backward, t = len-1 ... 0
  {
    DienCell<H, NH> g;
    g.load(w.Wg, w.bg, w.Wc, w.bc, p);
    DienCellT<H, NH, false> gt;
    gt.load(w.Wg, w.Wc, p);
    const float wj = wea[j];
    float dhc = 0.f;  // dL/dh_t carried down the chain
    float r = 0.f, u = 0.f, c = 0.f, hp = 0.f, dx = 0.f;
    const float* x = zero_row;
    if (len > 0) {
      const int t = len - 1;
      if (dxb) dx = dxb[t * NH + j];
      const long long o = offs[t];
      x = o >= 0 ? key_table + o : zero_row;
      float gi[NG], ci;
      g.input(x, gi, ci);
      hp = t > 0 ? hsb[(t - 1) * NH + j] : 0.f;
      g.gates(gi, ci, hp, half, r, u, c);
    }
    for (int t = len - 1; t >= 0; --t) {
      float rn = 0.f, un = 0.f, cn = 0.f, hpn = 0.f, dxn = 0.f;
      const float* xn = zero_row;
      if (t > 0) {
        if (dxb) dxn = dxb[(t - 1) * NH + j];  // loaded a step ahead, like the gates
        const long long o = offs[t - 1];
        xn = o >= 0 ? key_table + o : zero_row;
        float gi[NG], ci;
        g.input(xn, gi, ci);
        hpn = t > 1 ? hsb[(t - 2) * NH + j] : 0.f;
        g.gates(gi, ci, hpn, half, rn, un, cn);
      }
      float dht = dhc + fmaf(da[t], wj, dh[t * NH + j]);
      if (dxb) dht += dx;  // a branch, not an added zero: without d_hs the arithmetic is unchanged
      const float dc = fmaf(-u, dht, dht);
      const float dpu = dht * (hp - c) * u * (1.0f - u);
      const float dpc = dc * fmaf(-c, c, 1.0f);
      float unused = 0.f;
      const float drh = gt.cand(dpc, unused);
      const float dpr = drh * hp * r * (1.0f - r);
      const float back = gt.gate(dpr, dpu, half, unused);
      dhc = fmaf(u, dht, fmaf(drh, r, back));
      // off the chain: this step's rows of G1 / O1
      float* g1 = gr.g1 + (b * T + t) * LG;
      float* o1 = gr.o1 + (b * T + t) * LO1;
      if (p < NH) {
        g1[j] = dpr;
        g1[NH + j] = dpu;
        g1[2 * NH + j] = dpc;
        o1[H + j] = hp;
        o1[H + NH + j] = r * hp;
      }
      for (int i = p; i < H; i += 16) o1[i] = x[i];
      r = rn, u = un, c = cn, hp = hpn, x = xn, dx = dxn;
    }
  }
}

// One cell's weight gradients out of P = G^T O [3nh, XW + 2nh] and its row sums S [3nh]:
// dGw [2nh, XW + nh] = P[:2nh, :XW + nh], dGb = S[:2nh], dCw [nh, XW + nh] = P[2nh:, [x | r*state]], dCb = S[2nh:].
__global__ void dien_unpack_wgrad_kernel(const float* __restrict__ P, const float* __restrict__ S, int XW, int nh,
                                         float* dGw, float* dGb, float* dCw, float* dCb) {
  const int ldp = XW + 2 * nh, ldw = XW + nh;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < 3 * nh * ldw; e += gridDim.x * blockDim.x) {
    const int i = e / ldw, k = e % ldw;
    if (i < 2 * nh)
      dGw[i * ldw + k] = P[i * ldp + k];
    else
      dCw[(i - 2 * nh) * ldw + k] = P[i * ldp + (k < XW ? k : k + nh)];
    if (k == 0) (i < 2 * nh ? dGb[i] : dCb[i - 2 * nh]) = S[i];
  }
}

static int64_t align4(int64_t n) { return (n + 3) & ~(int64_t)3; }

struct DienBwdLayout {
  int64_t g1, o1, g2, o2, dwea, qc, prod, wgrad, wgrad_floats, total;
};

static DienBwdLayout dien_bwd_layout(int64_t batch, int T, int H, int nh) {
  const int64_t R = batch * T;
  DienBwdLayout l;
  int64_t at = 0;
  l.g1 = at, at += R * 3 * nh;
  l.o1 = at, at += R * (H + 2 * nh);
  l.g2 = at, at += R * 3 * nh;
  l.o2 = at, at += R * 3 * nh;
  l.dwea = at, at += batch * nh;
  l.qc = at, at += batch * H;
  const int X = H > nh ? H : nh;
  l.prod = at, at += 3 * nh * (X + 2 * nh) + 4 * nh;  // G^T O of one cell and its row sums
  l.wgrad = at;
  l.wgrad_floats = std::max(rk_gemm_wgrad_workspace_floats(3 * nh, X + 2 * nh, R), rk_gemm_wgrad_workspace_floats(nh, H, batch));
  l.total = align4(at + l.wgrad_floats);
  return l;
}

}  // namespace rk

using namespace rk;

RK_API int64_t rk_dien_interest_backward_workspace_floats(int64_t batch, int32_t T, int32_t H, int32_t nh) {
  if (batch <= 0 || T <= 0 || H <= 0 || nh <= 0) return 0;
  return dien_bwd_layout(batch, T, H, nh).total;
}

RK_API int rk_dien_interest_backward_aux(const float* query, int64_t ld_query, const float* keys, int64_t key_rows,
                                         int64_t ld_key, const int64_t* seq, int64_t ld_seq, int64_t ld_keys_b,
                                         int32_t T, const int64_t* seq_len, int64_t batch, int32_t H, int32_t nh,
                                         int32_t cell_type, const float* Wg, const float* bg, const float* Wc,
                                         const float* bc, const float* A, const float* Vg, const float* vg,
                                         const float* Vc, const float* vc, const float* hs, const float* ss,
                                         const float* att, int64_t ld_att, const float* d_out, int64_t ld_dout,
                                         float* dquery, int64_t ld_dquery, int32_t accumulate_dquery, float* dkeys,
                                         float* dWg, float* dbg, float* dWc, float* dbc, float* dA, float* dVg,
                                         float* dvg, float* dVc, float* dvc, int64_t* seq_masked, const float* d_hs,
                                         int32_t accumulate_dkeys, float* workspace, int64_t workspace_floats,
                                         void* stream) {
  const char* who = "rk_dien_interest_backward_aux";
  if (!query || !keys || !seq_len || !Wg || !bg || !Wc || !bc || !A || !Vg || !vg || !Vc || !vc || !hs || !ss ||
      !att || !d_out || !dquery || !dkeys || !dWg || !dbg || !dWc || !dbc || !dA || !dVg || !dvg || !dVc || !dvc)
    return fail(RK_ERR_INVALID, "%s: null pointer", who);
  if (T <= 0 || batch < 0 || H <= 0 || nh <= 0 || ld_query < H || ld_dout < nh || ld_dquery < H || ld_key < H ||
      ld_att < T || (seq && (key_rows <= 0 || ld_seq < T)) ||
      (!seq && ld_keys_b < (int64_t)T * ld_key && batch > 1))
    return fail(RK_ERR_INVALID, "%s: bad shape T=%d H=%d nh=%d", who, T, H, nh);
  if (int rc = dien_check_cell(who, cell_type)) return rc;
  if (int rc = dien_check_envelope(who, H, nh, T)) return rc;
  if (ld_key % 4 != 0 || ld_keys_b % 4 != 0 || (((uintptr_t)keys | (uintptr_t)hs | (uintptr_t)ss) & 15u))
    return fail(RK_ERR_UNSUPPORTED, "%s: history rows and saved states must be 16-B aligned", who);
  hipStream_t st = (hipStream_t)stream;
  const int ldw = H + nh;
  if (batch == 0) {  // no rows: every weight gradient is zero
    (void)hipMemsetAsync(dWg, 0, sizeof(float) * 2 * nh * ldw, st);
    (void)hipMemsetAsync(dbg, 0, sizeof(float) * 2 * nh, st);
    (void)hipMemsetAsync(dWc, 0, sizeof(float) * nh * ldw, st);
    (void)hipMemsetAsync(dbc, 0, sizeof(float) * nh, st);
    (void)hipMemsetAsync(dA, 0, sizeof(float) * nh * H, st);
    (void)hipMemsetAsync(dVg, 0, sizeof(float) * 4 * nh * nh, st);
    (void)hipMemsetAsync(dvg, 0, sizeof(float) * 2 * nh, st);
    (void)hipMemsetAsync(dVc, 0, sizeof(float) * 2 * nh * nh, st);
    (void)hipMemsetAsync(dvc, 0, sizeof(float) * nh, st);
    return check_launch(who);
  }
  const DienBwdLayout l = dien_bwd_layout(batch, T, H, nh);
  if (!workspace || ((uintptr_t)workspace & 15u) || workspace_floats < l.total)
    return fail(RK_ERR_INVALID, "%s: needs a 16-B aligned workspace of %lld floats, got %lld", who,
                (long long)l.total, (long long)workspace_floats);
  const DienWeights w{Wg, bg, Wc, bc, A, Vg, vg, Vc, vc};
  float *g1 = workspace + l.g1, *o1 = workspace + l.o1, *g2 = workspace + l.g2, *o2 = workspace + l.o2;
  const DienGrads gr{dquery, g1, o1, g2, o2, workspace + l.dwea, workspace + l.qc, seq_masked};
  // floats of LDS per sample: dh, da and att, wea and dwl, offs (see the kernel's carve-up)
  const int t4 = (T + 3) & ~3;
  const int stride = dien_padded_stride(T * nh + 2 * t4 + 32 + 2 * t4);
  const size_t shm = (size_t)(32 + kDienSamples * stride) * sizeof(float);
  const unsigned blocks = (unsigned)((batch + kDienSamples - 1) / kDienSamples);
  dien_launch(
      H, nh, [](auto s) { return dien_interest_backward_kernel<s.H, s.NH>; }, blocks, shm, st, query, ld_query, keys,
      key_rows, ld_key, seq, ld_seq, ld_keys_b, T, seq_len, batch, w, cell_type, stride, hs, ss, att, ld_att, d_out,
      ld_dout, ld_dquery, accumulate_dquery, gr, d_hs);
  int rc = check_launch(who);
  if (rc != RK_OK) return rc;
  const int64_t R = batch * T;
  const int lg = 3 * nh, lo1 = H + 2 * nh;
  float* ws = workspace + l.wgrad;
  const int64_t nws = l.wgrad_floats;
  // dkeys (+)= G1 . [Wg[:, :H]; Wc[:, :H]] (rows t >= len of G1 are zero, so are those of the product)
  if ((rc = rk_gemm(0, 1, R, H, 2 * nh, g1, lg, nullptr, Wg, ldw, dkeys, H, nullptr, accumulate_dkeys ? 1 : 0, 1, stream)) != RK_OK) return rc;
  if ((rc = rk_gemm(0, 1, R, H, nh, g1 + 2 * nh, lg, nullptr, Wc, ldw, dkeys, H, nullptr, 1, 1, stream)) != RK_OK) return rc;
  // One product per cell, P = G^T O [3nh, XW + 2nh] with its row sums (a call costs the same whatever
  // part of its 128 x 128 tile is used), then its blocks go to their places:
  // dWg = P[:2nh, [x|h']], dWc = P[2nh:, [x | r*h']]; the evolution the same with [h_t | s' | r*s'].
  float* P = workspace + l.prod;
  float* S = P + 3 * nh * ((H > nh ? H : nh) + 2 * nh);
  if ((rc = rk_gemm_wgrad(lg, lo1, R, g1, lg, nullptr, o1, lo1, P, lo1, S, 0, ws, nws, stream)) != RK_OK) return rc;
  dien_unpack_wgrad_kernel<<<4, 256, 0, st>>>(P, S, H, nh, dWg, dbg, dWc, dbc);
  if ((rc = rk_gemm_wgrad(lg, lg, R, g2, lg, nullptr, o2, lg, P, lg, S, 0, ws, nws, stream)) != RK_OK) return rc;
  dien_unpack_wgrad_kernel<<<4, 256, 0, st>>>(P, S, nh, nh, dVg, dvg, dVc, dvc);
  if ((rc = check_launch(who)) != RK_OK) return rc;
  // dA = d(A q)^T q
  return rk_gemm_wgrad(nh, H, batch, workspace + l.dwea, nh, nullptr, workspace + l.qc, H, dA, H, nullptr, 0, ws, nws, stream);
}

RK_API int rk_dien_interest_backward(const float* query, int64_t ld_query, const float* keys, int64_t key_rows,
                                     int64_t ld_key, const int64_t* seq, int64_t ld_seq, int64_t ld_keys_b, int32_t T,
                                     const int64_t* seq_len, int64_t batch, int32_t H, int32_t nh, int32_t cell_type,
                                     const float* Wg, const float* bg, const float* Wc, const float* bc,
                                     const float* A, const float* Vg, const float* vg, const float* Vc,
                                     const float* vc, const float* hs, const float* ss, const float* att,
                                     int64_t ld_att, const float* d_out, int64_t ld_dout, float* dquery,
                                     int64_t ld_dquery, int32_t accumulate_dquery, float* dkeys, float* dWg,
                                     float* dbg, float* dWc, float* dbc, float* dA, float* dVg, float* dvg,
                                     float* dVc, float* dvc, int64_t* seq_masked, float* workspace,
                                     int64_t workspace_floats, void* stream) {
  return rk_dien_interest_backward_aux(query, ld_query, keys, key_rows, ld_key, seq, ld_seq, ld_keys_b, T, seq_len,
                                       batch, H, nh, cell_type, Wg, bg, Wc, bc, A, Vg, vg, Vc, vc, hs, ss, att, ld_att,
                                       d_out, ld_dout, dquery, ld_dquery, accumulate_dquery, dkeys, dWg, dbg, dWc, dbc,
                                       dA, dVg, dvg, dVc, dvc, seq_masked, nullptr, 0, workspace, workspace_floats,
                                       stream);
}
