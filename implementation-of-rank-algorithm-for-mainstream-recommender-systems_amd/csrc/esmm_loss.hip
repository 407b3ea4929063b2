// ESMM's entire-space loss with its analytic gradient, and the fold of gradients arriving at the joint
// probabilities back onto the conditional logits.
//
//   rk_esmm_loss            per row, with ls_j = logsigmoid(z_j) and S_k = ls_0 + ... + ls_k = log prob_k:
//                             L_0 = softplus(-z_0) y_0 + softplus(z_0) (1 - y_0)
//                             L_k = -(y_k S_k + (1 - y_k) log1mexp(S_k)),  k >= 1
//                           in the log domain: the product of sigmoids and 1 - pq are never formed, so the
//                           loss and its gradient stay exact when logits saturate.  Two
//                           launches: one thread per row (the gradient, and per workgroup the sums of its
//                           256 rows per task, a fixed butterfly / tree), then one workgroup that adds the
//                           workgroups' sums in a fixed order in double.  No atomics.
//   rk_esmm_joint_backward  g_j = dlogits_j + s(z_j) s(-z_j) dcond_j + s(-z_j) sum_{k >= j} dprobs_k prob_k
//                           (d prob_k / d z_j = prob_k s(-z_j) for j <= k: no division by a probability)
//
// Rows are independent; both kernels are memory-bound and read each value once.
#include <cfloat>

#include "common.h"

namespace rk {

constexpr int kLossMaxTasks = 8;
constexpr int kLossRows = 256;  // rows (threads) per workgroup

struct LossWeights {
  float w[kLossMaxTasks];
};

__device__ __forceinline__ float softplus_f(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// sigmoid(-x), relative accuracy kept where it is tiny
__device__ __forceinline__ float sigmoid_neg(float x) {
  const float e = expf(-fabsf(x));
  return x >= 0.f ? e / (1.f + e) : 1.f / (1.f + e);
}

// log(1 - exp(s)), s < 0
__device__ __forceinline__ float log1mexp_f(float s) {
  return s > -0.69314718f ? logf(-expm1f(s)) : log1pf(-expf(s));
}

__global__ __launch_bounds__(kLossRows) void esmm_loss_kernel(int64_t batch, int K, const float* __restrict__ logits,
                                                              int64_t ld_z, const float* __restrict__ labels,
                                                              int64_t ld_y, LossWeights w, float inv_batch,
                                                              float* __restrict__ dlogits, int64_t ld_d,
                                                              float* __restrict__ partial) {
  __shared__ float part[kLossRows / 64][kLossMaxTasks];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = (int64_t)blockIdx.x * kLossRows + tid;
  float L[kLossMaxTasks];
#pragma unroll
  for (int k = 0; k < kLossMaxTasks; ++k) L[k] = 0.f;
  if (b < batch) {
    float sn[kLossMaxTasks], em[kLossMaxTasks], y[kLossMaxTasks];
    float S = 0.f;
#pragma unroll
    for (int k = 0; k < kLossMaxTasks; ++k) {
      sn[k] = em[k] = y[k] = 0.f;
      if (k < K) {
        const float z = logits[b * ld_z + k];
        y[k] = labels[b * ld_y + k];
        sn[k] = sigmoid_neg(z);
        S -= softplus_f(-z);
        if (k == 0) {
          L[0] = softplus_f(-z) * y[0] + softplus_f(z) * (1.f - y[0]);
        } else {
          const float Sc = fminf(S, -FLT_MIN);
          L[k] = -(y[k] * S + (1.f - y[k]) * log1mexp_f(Sc));
          em[k] = expm1f(-Sc);
        }
      }
    }
    if (dlogits) {
#pragma unroll
      for (int j = 0; j < kLossMaxTasks; ++j) {
        if (j < K) {
          // sigma(-z_j) / expm1(-S_k) <= sigma(z_j) for k >= j: each term is bounded, the sum of the
          // unscaled quotients is not, so the product is taken term by term
          float g = j == 0 ? ((1.f - sn[0]) - y[0]) * w.w[0] : 0.f;
#pragma unroll
          for (int k = 1; k < kLossMaxTasks; ++k)
            if (k >= j && k < K) g += w.w[k] * ((sn[j] * (1.f - y[k])) / em[k] - sn[j] * y[k]);
          dlogits[b * ld_d + j] = g * inv_batch;
        }
      }
    }
  }
  // the workgroup's sums per task: the wave butterfly, then the waves in ascending order
#pragma unroll
  for (int k = 0; k < kLossMaxTasks; ++k) {
    const float s = wave_sum(L[k]);
    if (lane == 0) part[wave][k] = s;
  }
  __syncthreads();
  if (tid < kLossMaxTasks) {
    float s = 0.f;
    for (int i = 0; i < kLossRows / 64; ++i) s += part[i][tid];
    partial[(int64_t)blockIdx.x * kLossMaxTasks + tid] = s;
  }
}

// One workgroup: per task, thread t adds the workgroups t, t + 256, ... in ascending order, then a tree.
__global__ __launch_bounds__(256) void esmm_loss_finish_kernel(int64_t blocks, int K, const float* __restrict__ partial,
                                                               LossWeights w, double inv_batch,
                                                               float* __restrict__ loss, float* __restrict__ per_task) {
  __shared__ double acc[256];
  __shared__ double mean[kLossMaxTasks];
  const int tid = threadIdx.x;
  for (int k = 0; k < K; ++k) {
    double s = 0.0;
    for (int64_t i = tid; i < blocks; i += 256) s += (double)partial[i * kLossMaxTasks + k];
    acc[tid] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
      if (tid < h) acc[tid] += acc[tid + h];
      __syncthreads();
    }
    if (tid == 0) mean[k] = acc[0] * inv_batch;
    __syncthreads();
  }
  if (tid == 0) {
    double total = 0.0;
    for (int k = 0; k < K; ++k) {
      total += (double)w.w[k] * mean[k];
      if (per_task) per_task[k] = (float)mean[k];
    }
    if (loss) *loss = (float)total;
  }
}

__global__ __launch_bounds__(256) void esmm_joint_backward_kernel(int64_t batch, int K, const float* __restrict__ logits,
                                                                  int64_t ld_z, const float* __restrict__ dlogits,
                                                                  const float* __restrict__ dprobs,
                                                                  const float* __restrict__ dcond, int64_t ld_in,
                                                                  float* __restrict__ g, int64_t ld_g) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= batch) return;
  float c[kLossMaxTasks], sn[kLossMaxTasks], t[kLossMaxTasks];
  float run = 1.f;
#pragma unroll
  for (int k = 0; k < kLossMaxTasks; ++k) {
    c[k] = sn[k] = t[k] = 0.f;
    if (k < K) {
      sn[k] = sigmoid_neg(logits[b * ld_z + k]);
      c[k] = 1.f - sn[k];
      run *= c[k];
      t[k] = dprobs ? dprobs[b * ld_in + k] * run : 0.f;
    }
  }
  float tail = 0.f;  // sum_{k >= j} dprobs_k prob_k, k descending
#pragma unroll
  for (int j = kLossMaxTasks - 1; j >= 0; --j) {
    if (j < K) {
      tail += t[j];
      float v = sn[j] * tail;
      if (dlogits) v += dlogits[b * ld_in + j];
      if (dcond) v += c[j] * sn[j] * dcond[b * ld_in + j];
      g[b * ld_g + j] = v;
    }
  }
}

}  // namespace rk

using namespace rk;

namespace {
bool float_aligned(const void* p) { return ((uintptr_t)p & 3u) == 0; }
}  // namespace

RK_API int64_t rk_esmm_loss_workspace_floats(int64_t batch) {
  return batch <= 0 ? kLossMaxTasks : (batch + kLossRows - 1) / kLossRows * kLossMaxTasks;
}

RK_API int rk_esmm_loss(const float* logits, int64_t ld_logits, const float* labels, int64_t ld_labels, int64_t batch,
                        int32_t num_tasks, const float* task_weights, float* loss, float* per_task, float* dlogits,
                        int64_t ld_dlogits, float* workspace, int64_t workspace_floats, void* stream) {
  if (batch < 0 || num_tasks <= 0 || (batch > 0 && (!logits || !labels)) || (!loss && !per_task && !dlogits) || !workspace)
    return fail(RK_ERR_INVALID, "rk_esmm_loss: null pointer or negative size (batch %lld)", (long long)batch);
  if (num_tasks > kLossMaxTasks)
    return fail(RK_ERR_UNSUPPORTED, "rk_esmm_loss: %d tasks (<= %d)", num_tasks, kLossMaxTasks);
  if (ld_logits < num_tasks || ld_labels < num_tasks || (dlogits && ld_dlogits < num_tasks) ||
      workspace_floats < rk_esmm_loss_workspace_floats(batch))
    return fail(RK_ERR_INVALID, "rk_esmm_loss: a leading dimension below num_tasks or a short workspace");
  if (!float_aligned(logits) || !float_aligned(labels) || !float_aligned(loss) || !float_aligned(per_task) ||
      !float_aligned(dlogits) || !float_aligned(workspace))
    return fail(RK_ERR_INVALID, "rk_esmm_loss: pointer not aligned to a float");
  LossWeights w;
  for (int k = 0; k < kLossMaxTasks; ++k) w.w[k] = k < num_tasks ? (task_weights ? task_weights[k] : 1.f) : 0.f;
  const int64_t blocks = (batch + kLossRows - 1) / kLossRows;
  if (blocks > INT32_MAX) return fail(RK_ERR_UNSUPPORTED, "rk_esmm_loss: batch too large");
  const double inv = batch > 0 ? 1.0 / (double)batch : 0.0;
  if (batch > 0) {
    esmm_loss_kernel<<<(unsigned)blocks, kLossRows, 0, (hipStream_t)stream>>>(
        batch, num_tasks, logits, ld_logits, labels, ld_labels, w, (float)inv, dlogits, ld_dlogits, workspace);
    if (int rc = check_launch("rk_esmm_loss")) return rc;
  }
  if (loss || per_task) {
    esmm_loss_finish_kernel<<<1, 256, 0, (hipStream_t)stream>>>(blocks, num_tasks, workspace, w, inv, loss, per_task);
    return check_launch("rk_esmm_loss");
  }
  return RK_OK;
}

RK_API int rk_esmm_joint_backward(const float* logits, int64_t ld_logits, const float* dlogits, const float* dprobs,
                                  const float* dcond, int64_t ld_in, int64_t batch, int32_t num_tasks, float* g,
                                  int64_t ld_g, void* stream) {
  if (batch < 0 || num_tasks <= 0 || !logits || !g || (!dlogits && !dprobs && !dcond) || ld_logits < num_tasks ||
      ld_in < num_tasks || ld_g < num_tasks)
    return fail(RK_ERR_INVALID, "rk_esmm_joint_backward: null pointer, no incoming gradient or a leading dimension "
                "below num_tasks");
  if (num_tasks > kLossMaxTasks)
    return fail(RK_ERR_UNSUPPORTED, "rk_esmm_joint_backward: %d tasks (<= %d)", num_tasks, kLossMaxTasks);
  if (!float_aligned(logits) || !float_aligned(dlogits) || !float_aligned(dprobs) || !float_aligned(dcond) ||
      !float_aligned(g))
    return fail(RK_ERR_INVALID, "rk_esmm_joint_backward: pointer not aligned to a float");
  if (batch == 0) return RK_OK;
  const int64_t blocks = (batch + 255) / 256;
  if (blocks > INT32_MAX) return fail(RK_ERR_UNSUPPORTED, "rk_esmm_joint_backward: batch too large");
  esmm_joint_backward_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(batch, num_tasks, logits, ld_logits,
                                                                               dlogits, dprobs, dcond, ld_in, g, ld_g);
  return check_launch("rk_esmm_joint_backward");
}
