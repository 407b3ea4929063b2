// MMoE training backward: the two kernels between the grouped Linear backwards (rk_gemm_grouped,
// rk_gemm_wgrad_grouped) that are MMoE's own.
//
//   rk_mmoe_mix_backward   the mix m_k = sum_e g_k[e] f_e and the gates' softmax, one wave per row:
//                            dg[k][e]  = sum_h dmixed[k][h] f_e[h]
//                            dgl[k][e] = g[k][e] (dg[k][e] - sum_e' g[k][e'] dg[k][e'])   -> the gate logits
//                            dz_e[h]   = (sum_k g[k][e] dmixed[k][h]) [f_e[h] > 0] mask_scale
//                          f_e is the expert's last output after ReLU and dropout, so f_e > 0 holds
//                          exactly where the element was kept and its pre-activation positive: dz_e
//                          is the gradient of the last pre-activation, masked once.
//   rk_mmoe_head_backward  the K heads (Linear(n, 1) + sigmoid): g[b][k] = dlogit + dprob p (1 - p) and
//                          dt_k = g w_k, masked by the tower's last output like dz_e.  The heads' weight
//                          and bias gradients are one rk_gemm_wgrad of g^T [K, B] against the towers'
//                          side-by-side outputs (its diagonal blocks), so nothing here sums over rows.
//
// Rows are independent and every sum runs in a fixed order (h: lane-strided partial sums folded by
// wave_sum's butterfly; k and e' ascending): no atomics, two runs give the same bits.  Both kernels
// are memory-bound; f and dmixed of a row are re-read from L1 / L2 per (k, e) pair instead of staged.
#include "common.h"

namespace rk {

constexpr int kMixMaxExperts = 16;
constexpr int kMixMaxTasks = 8;
constexpr int kMixMaxGates = 64;  // tasks x experts: one lane each
constexpr int kMixMaxH = 512;
constexpr int kMixRows = 4;       // waves (rows) per workgroup

__global__ __launch_bounds__(64 * kMixRows) void mmoe_mix_backward_kernel(
    int64_t batch, int E, int K, int H, const float* __restrict__ dmixed, int64_t ld_dm, int pitch_dm,
    const float* __restrict__ f, int64_t ld_f, int pitch_f, const float* __restrict__ gate_probs, float mask_scale,
    float* __restrict__ dgl, int64_t ld_dgl, float* __restrict__ dz, int64_t ld_dz, int pitch_dz) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * kMixRows + (threadIdx.x >> 6);
  if (b >= batch) return;  // (whole waves; no barrier below)
  const float* dm = dmixed + b * ld_dm;
  const float* fr = f + b * ld_f;
  const float gv = lane < K * E ? gate_probs[b * K * E + lane] : 0.f;  // lane k E + e holds g[k][e]
  // the gate logits' gradient, task by task
  for (int k = 0; k < K; ++k) {
    float dg[kMixMaxExperts];
#pragma unroll
    for (int e = 0; e < kMixMaxExperts; ++e) {
      dg[e] = 0.f;
      if (e < E) {
        float p = 0.f;
        for (int h = lane; h < H; h += 64) p = fmaf(dm[k * pitch_dm + h], fr[e * pitch_f + h], p);
        dg[e] = wave_sum(p);
      }
    }
    float s = 0.f, mine = 0.f, gmine = 0.f;
#pragma unroll
    for (int e = 0; e < kMixMaxExperts; ++e)
      if (e < E) {
        const float g = __shfl(gv, k * E + e, kWave);
        s = fmaf(g, dg[e], s);
        if (lane == e) {
          mine = dg[e];
          gmine = g;
        }
      }
    if (lane < E) dgl[b * ld_dgl + k * E + lane] = gmine * (mine - s);
  }
  // the experts' last pre-activations (zeros up to the pitch)
  for (int e = 0; e < E; ++e) {
    float ge[kMixMaxTasks];  // g[k][e], read from its lane while the whole wave is active
#pragma unroll
    for (int k = 0; k < kMixMaxTasks; ++k) ge[k] = k < K ? __shfl(gv, k * E + e, kWave) : 0.f;
    for (int h = lane; h < pitch_dz; h += 64) {
      float v = 0.f;
      if (h < H && fr[e * pitch_f + h] > 0.f) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < kMixMaxTasks; ++k)
          if (k < K) t = fmaf(ge[k], dm[k * pitch_dm + h], t);
        v = t * mask_scale;
      }
      dz[b * ld_dz + e * pitch_dz + h] = v;
    }
  }
}

constexpr int kHeadBwdRows = 16;
constexpr int kHeadBwdMaxTasks = 8;
struct HeadWeights {
  const float* w[kHeadBwdMaxTasks];
};

__global__ __launch_bounds__(256) void mmoe_head_backward_kernel(
    int64_t batch, int K, int n, int pitch, const float* __restrict__ dlogits, const float* __restrict__ dprobs,
    const float* __restrict__ probs, HeadWeights hw, const float* __restrict__ t, float mask_scale,
    float* __restrict__ g_out, int ld_g, float* __restrict__ dt, int accumulate) {
  __shared__ float gs[kHeadBwdRows * kHeadBwdMaxTasks];
  const int tid = threadIdx.x;
  const int64_t b0 = (int64_t)blockIdx.x * kHeadBwdRows;
  const int rows = (int)min<int64_t>(kHeadBwdRows, batch - b0);
  if (tid < kHeadBwdRows * kHeadBwdMaxTasks) {
    const int row = tid / kHeadBwdMaxTasks, k = tid % kHeadBwdMaxTasks;
    float g = 0.f;
    if (row < rows && k < K) {
      const int64_t i = (b0 + row) * K + k;
      if (dlogits) g = dlogits[i];
      if (dprobs) {
        const float p = probs[i];
        g += dprobs[i] * (1.f - p) * p;  // sigmoid_backward: grad * (1 - y) * y
      }
    }
    gs[tid] = g;
    if (row < rows && k < ld_g) g_out[(b0 + row) * ld_g + k] = g;  // zeros up to the pitch
  }
  __syncthreads();
  const int ld = K * pitch;
  for (int i = tid; i < rows * ld; i += 256) {
    const int row = i / ld, c = i - row * ld;
    const int k = c / pitch, j = c - k * pitch;
    const int64_t o = (b0 + row) * ld + c;
    float v = 0.f;
    if (j < n) {
      v = gs[row * kHeadBwdMaxTasks + k] * hw.w[k][j];
      if (t) v = t[o] > 0.f ? v * mask_scale : 0.f;
    }
    dt[o] = accumulate ? dt[o] + v : v;
  }
}

}  // namespace rk

using namespace rk;

RK_API int rk_mmoe_mix_backward(int64_t batch, int32_t num_experts, int32_t num_tasks, int32_t H, const float* dmixed,
                                int64_t ld_dmixed, int32_t pitch_dmixed, const float* f, int64_t ld_f, int32_t pitch_f,
                                const float* gate_probs, float mask_scale, float* dgate_logits, int64_t ld_dgl,
                                float* dz, int64_t ld_dz, int32_t pitch_dz, void* stream) {
  if (batch < 0 || num_experts <= 0 || num_tasks <= 0 || H <= 0 || !dmixed || !f || !gate_probs || !dgate_logits ||
      !dz)
    return fail(RK_ERR_INVALID, "rk_mmoe_mix_backward: null pointer or non-positive size");
  if (num_experts > kMixMaxExperts || num_tasks > kMixMaxTasks || num_tasks * num_experts > kMixMaxGates ||
      H > kMixMaxH)
    return fail(RK_ERR_UNSUPPORTED, "rk_mmoe_mix_backward: %d experts (<= %d), %d tasks (<= %d, tasks x experts <= "
                                    "%d), H %d (<= %d)",
                num_experts, kMixMaxExperts, num_tasks, kMixMaxTasks, kMixMaxGates, H, kMixMaxH);
  if (pitch_dmixed < H || pitch_f < H || pitch_dz < H || ld_dmixed < (int64_t)(num_tasks - 1) * pitch_dmixed + H ||
      ld_f < (int64_t)(num_experts - 1) * pitch_f + H || ld_dz < (int64_t)num_experts * pitch_dz ||
      ld_dgl < (int64_t)num_tasks * num_experts)
    return fail(RK_ERR_INVALID, "rk_mmoe_mix_backward: pitch / leading dimension too small");
  if (((uintptr_t)dmixed | (uintptr_t)f | (uintptr_t)gate_probs | (uintptr_t)dgate_logits | (uintptr_t)dz) & 3)
    return fail(RK_ERR_INVALID, "rk_mmoe_mix_backward: pointer not aligned to a float");
  if (batch == 0) return RK_OK;
  const int64_t blocks = (batch + kMixRows - 1) / kMixRows;
  if (blocks > INT32_MAX) return fail(RK_ERR_UNSUPPORTED, "rk_mmoe_mix_backward: batch too large");
  mmoe_mix_backward_kernel<<<(unsigned)blocks, 64 * kMixRows, 0, (hipStream_t)stream>>>(
      batch, num_experts, num_tasks, H, dmixed, ld_dmixed, pitch_dmixed, f, ld_f, pitch_f, gate_probs, mask_scale,
      dgate_logits, ld_dgl, dz, ld_dz, pitch_dz);
  return check_launch("rk_mmoe_mix_backward");
}

RK_API int rk_mmoe_head_backward(int64_t batch, int32_t num_tasks, int32_t n, int32_t pitch, const float* dlogits,
                                 const float* dprobs, const float* probs, const float* const* head_w, const float* t,
                                 float mask_scale, float* g_out, int32_t ld_g, float* dt, int32_t accumulate,
                                 void* stream) {
  if (batch < 0 || num_tasks <= 0 || n <= 0 || pitch < n || !head_w || !g_out || !dt || ld_g < num_tasks ||
      (dprobs && !probs) || (!dlogits && !dprobs))
    return fail(RK_ERR_INVALID, "rk_mmoe_head_backward: null pointer or bad size");
  if (num_tasks > kHeadBwdMaxTasks || ld_g > kHeadBwdMaxTasks)
    return fail(RK_ERR_UNSUPPORTED, "rk_mmoe_head_backward: %d tasks (<= %d)", num_tasks, kHeadBwdMaxTasks);
  HeadWeights hw = {};
  for (int k = 0; k < num_tasks; ++k) {
    if (!head_w[k] || ((uintptr_t)head_w[k] & 3)) return fail(RK_ERR_INVALID, "rk_mmoe_head_backward: head %d null", k);
    hw.w[k] = head_w[k];
  }
  if (((uintptr_t)dlogits | (uintptr_t)dprobs | (uintptr_t)probs | (uintptr_t)t | (uintptr_t)g_out | (uintptr_t)dt) & 3)
    return fail(RK_ERR_INVALID, "rk_mmoe_head_backward: pointer not aligned to a float");
  if (batch == 0) return RK_OK;
  const int64_t blocks = (batch + kHeadBwdRows - 1) / kHeadBwdRows;
  if (blocks > INT32_MAX) return fail(RK_ERR_UNSUPPORTED, "rk_mmoe_head_backward: batch too large");
  mmoe_head_backward_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(
      batch, num_tasks, n, pitch, dlogits, dprobs, probs, hw, t, mask_scale, g_out, ld_g, dt, accumulate);
  return check_launch("rk_mmoe_head_backward");
}
