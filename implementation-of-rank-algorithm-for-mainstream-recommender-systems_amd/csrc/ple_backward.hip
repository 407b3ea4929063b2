// PLE training backward: the kernel between the grouped Linear backwards (rk_gemm_grouped,
// rk_gemm_wgrad_grouped) that is PLE's own, the mixtures and gates of one extraction level.
//
// A level has K task gates over ms + mc columns and, unless it is the last, a shared gate over all NE =
// K ms + mc stacks; nq = K (+ 1) mixtures.  s(i, c), the stack behind column c of gate i, is
// i ms + c (c < ms) or K ms + c - ms for a task gate and c for the shared one.  Per row, with dm_i the
// gradient of mixture i, f_s the saved last layer of stack s (after ReLU and dropout) and g_i the gate's
// softmax weights:
//   dg_i[c]  = sum_h dm_i[h] f_{s(i,c)}[h]
//   dgl_i[c] = g_i[c] (dg_i[c] - sum_c' g_i[c'] dg_i[c'])                        -> the gate's logits
//   dz_s[h]  = (sum over the (i, c) with s(i, c) = s, i ascending, of g_i[c] dm_i[h]) mask_scale [f_s[h] > 0]
// f_s > 0 holds exactly where the element was kept and its pre-activation positive, so dz_s is the
// gradient of the stack's last pre-activation, masked once.
//
// One wave per row, H across the lanes (element h = lane + 64 e, at most 8 per lane).  The row's nq
// mixture gradients stay in registers (72 at most); the wave then walks the stacks once, s ascending:
// f_s is read once and used for every mixture the stack belongs to (a task's stack: its task's and the
// shared one; a shared stack: all nq), where rk_mmoe_mix_backward re-reads f and dmixed per (k, e) pair.
// dg_i[c] is left in lane c's register of gate i, so the softmax backward that follows is one wave_sum
// per gate with no memory in between.  The loops over the mixtures are unrolled over the envelope's 9
// with uniform predicates: a runtime index into the register rows would send them to scratch.
//
// Rows are independent and every sum runs in a fixed order (h: the lane's elements ascending, then
// wave_sum's butterfly; the columns of a gate by the same butterfly; i ascending): no atomics, two runs
// give the same bits.  A one-column gate has g = 1, so its dgl is dg - dg = 0 exactly.
//
// dgl_i goes to column gate_off[i] and dz_s to column stack_off[s] of their output rows, both with zeros
// up to the next multiple of 4 (dz: up to pitch_dz), so that the caller can place them inside the stacked
// layer-0 buffers of the level (ops.ple_backward) without a copy.
#include "common.h"

namespace rk {

constexpr int kPmMaxTasks = 8;
constexpr int kPmMaxMix = kPmMaxTasks + 1;
constexpr int kPmMaxStacks = 64;
constexpr int kPmMaxH = 512;
constexpr int kPmElems = kPmMaxH / 64;  // elements of a row per lane
constexpr int kPmRows = 4;              // waves (rows) per workgroup

struct PleMixArgs {
  int64_t batch;
  int K, ms, mc, nq, H;
  const float* dm;
  int64_t ld_dm;
  int pitch_dm;
  const float* f;
  int64_t ld_f;
  int pitch_f;
  const float* gates;
  int64_t ld_g;
  float mask_scale;
  float* dgl;
  int64_t ld_dgl;
  float* dz;
  int64_t ld_dz;
  int pitch_dz;
  int gate_off[kPmMaxMix];
  int stack_off[kPmMaxStacks];
};

__global__ __launch_bounds__(64 * kPmRows) void ple_mix_backward_kernel(PleMixArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * kPmRows + (threadIdx.x >> 6);
  if (b >= a.batch) return;  // (whole waves; no barrier below)
  const int K = a.K, ms = a.ms, mc = a.mc, nq = a.nq, H = a.H;
  const int NE = K * ms + mc, GT = ms + mc;
  const float* __restrict__ dmr = a.dm + b * a.ld_dm;
  const float* __restrict__ fr = a.f + b * a.ld_f;
  const float* __restrict__ gr = a.gates + b * a.ld_g;
  const int so = lane < NE ? a.stack_off[lane] : 0;  // lane s holds stack s's output column

  float dm[kPmMaxMix][kPmElems];
#pragma unroll
  for (int i = 0; i < kPmMaxMix; ++i)
#pragma unroll
    for (int e = 0; e < kPmElems; ++e) {
      const int h = lane + 64 * e;
      dm[i][e] = i < nq && h < H ? dmr[i * a.pitch_dm + h] : 0.f;
    }
  float dg[kPmMaxMix];  // dg[i]: lane c holds dg_i[c]
#pragma unroll
  for (int i = 0; i < kPmMaxMix; ++i) dg[i] = 0.f;

  for (int s = 0; s < NE; ++s) {
    const int owner = s < K * ms ? s / ms : K;
    float fs[kPmElems], t[kPmElems];
#pragma unroll
    for (int e = 0; e < kPmElems; ++e) {
      const int h = lane + 64 * e;
      fs[e] = h < H ? fr[s * a.pitch_f + h] : 0.f;
      t[e] = 0.f;
    }
#pragma unroll
    for (int i = 0; i < kPmMaxMix; ++i) {
      // (uniform: whether mixture i takes stack s, and through which column of its gate)
      int c = -1, goff = 0;
      if (i < K) {
        goff = i * GT;
        if (owner == i) c = s - i * ms;
        if (owner == K) c = ms + s - K * ms;
      } else if (i == K && nq > K) {
        goff = K * GT;
        c = s;
      }
      if (c >= 0) {
        const float g = gr[goff + c];
        float p = 0.f;
#pragma unroll
        for (int e = 0; e < kPmElems; ++e) {
          p = fmaf(dm[i][e], fs[e], p);
          t[e] = fmaf(g, dm[i][e], t[e]);
        }
        p = wave_sum(p);
        if (lane == c) dg[i] = p;
      }
    }
    float* const out = a.dz + b * a.ld_dz + __shfl(so, s, kWave);
#pragma unroll
    for (int e = 0; e < kPmElems; ++e) {
      const int h = lane + 64 * e;
      if (h < a.pitch_dz) out[h] = h < H && fs[e] > 0.f ? t[e] * a.mask_scale : 0.f;
    }
  }

  // the gates' softmax backward: gate i's n columns across the lanes
#pragma unroll
  for (int i = 0; i < kPmMaxMix; ++i) {
    if (i < nq) {
      const int n = i < K ? GT : NE, goff = i < K ? i * GT : K * GT;
      const float g = lane < n ? gr[goff + lane] : 0.f;
      const float sum = wave_sum(g * dg[i]);
      if (lane < ((n + 3) & ~3)) a.dgl[b * a.ld_dgl + a.gate_off[i] + lane] = lane < n ? g * (dg[i] - sum) : 0.f;
    }
  }
}

}  // namespace rk

using namespace rk;

RK_API int rk_ple_mix_backward(int64_t batch, int32_t num_tasks, int32_t num_specific, int32_t num_shared,
                               int32_t has_shared_mix, int32_t H, const float* dm, int64_t ld_dm, int32_t pitch_dm,
                               const float* f, int64_t ld_f, int32_t pitch_f, const float* gates, int64_t ld_gates,
                               float mask_scale, float* dgate_logits, int64_t ld_dgl, const int32_t* gate_offsets,
                               float* dz, int64_t ld_dz, const int32_t* stack_offsets, int32_t pitch_dz,
                               void* stream) {
  const char* const name = "rk_ple_mix_backward";
  if (batch < 0 || num_tasks <= 0 || num_specific < 0 || num_shared <= 0 || H <= 0 || !dm || !f || !gates ||
      !dgate_logits || !gate_offsets || !dz || !stack_offsets)
    return fail(RK_ERR_INVALID, "%s: null pointer or bad size (batch %lld)", name, (long long)batch);
  const int K = num_tasks, ms = num_specific, mc = num_shared;
  const int64_t NE = (int64_t)K * ms + mc;
  if (K > kPmMaxTasks || ms > kPmMaxStacks || mc > kPmMaxStacks || NE > kPmMaxStacks || H > kPmMaxH)
    return fail(RK_ERR_UNSUPPORTED, "%s: %d tasks (<= %d), %d specific and %d shared experts (tasks x specific + shared "
                "<= %d), H %d (<= %d)", name, K, kPmMaxTasks, ms, mc, kPmMaxStacks, H, kPmMaxH);
  const int nq = has_shared_mix ? K + 1 : K, GT = ms + mc;
  const int64_t gcols = (int64_t)K * GT + (has_shared_mix ? NE : 0);
  if (pitch_dm < H || pitch_f < H || pitch_dz < H || pitch_dz > kPmMaxH || ld_dm < (int64_t)(nq - 1) * pitch_dm + H ||
      ld_f < (NE - 1) * pitch_f + H || ld_gates < gcols)
    return fail(RK_ERR_INVALID, "%s: pitch / leading dimension too small", name);
  PleMixArgs a = {};
  for (int i = 0; i < nq; ++i) {
    const int n = i < K ? GT : (int)NE;
    if (gate_offsets[i] < 0 || (int64_t)gate_offsets[i] + (n + 3) / 4 * 4 > ld_dgl)
      return fail(RK_ERR_INVALID, "%s: gate %d at column %d does not fit a row of %lld", name, i, gate_offsets[i],
                  (long long)ld_dgl);
    a.gate_off[i] = gate_offsets[i];
  }
  for (int s = 0; s < NE; ++s) {
    if (stack_offsets[s] < 0 || (int64_t)stack_offsets[s] + pitch_dz > ld_dz)
      return fail(RK_ERR_INVALID, "%s: stack %d at column %d does not fit a row of %lld", name, s, stack_offsets[s],
                  (long long)ld_dz);
    a.stack_off[s] = stack_offsets[s];
  }
  if (((uintptr_t)dm | (uintptr_t)f | (uintptr_t)gates | (uintptr_t)dgate_logits | (uintptr_t)dz) & 3)
    return fail(RK_ERR_INVALID, "%s: pointer not aligned to a float", name);
  if (batch == 0) return RK_OK;
  const int64_t blocks = (batch + kPmRows - 1) / kPmRows;
  if (blocks > INT32_MAX) return fail(RK_ERR_UNSUPPORTED, "%s: batch too large", name);
  a.batch = batch;
  a.K = K;
  a.ms = ms;
  a.mc = mc;
  a.nq = nq;
  a.H = H;
  a.dm = dm;
  a.ld_dm = ld_dm;
  a.pitch_dm = pitch_dm;
  a.f = f;
  a.ld_f = ld_f;
  a.pitch_f = pitch_f;
  a.gates = gates;
  a.ld_g = ld_gates;
  a.mask_scale = mask_scale;
  a.dgl = dgate_logits;
  a.ld_dgl = ld_dgl;
  a.dz = dz;
  a.ld_dz = ld_dz;
  a.pitch_dz = pitch_dz;
  ple_mix_backward_kernel<<<(unsigned)blocks, 64 * kPmRows, 0, (hipStream_t)stream>>>(a);
  return check_launch(name);
}
