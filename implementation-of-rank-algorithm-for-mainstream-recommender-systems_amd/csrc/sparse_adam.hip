// Lazy (sparse) Adam over embedding tables: torch.optim.SparseAdam / TF LazyAdamOptimizer
// (DIEN/dien.py:328) for sparse COO gradients, every table of a step in one call.
//
//   for every distinct row r of a table's gradient:  g = sum of the row's entries (list order)
//     m += (1 - beta1) (g - m);  v += (1 - beta2) (g^2 - v)
//     p -= lr sqrt(1 - beta2^t) / (1 - beta1^t) * m / (sqrt(v) + eps)
//   rows that are not in the gradient are neither read nor written.
//
// The tables of a call are packed into groups of up to kSaMaxTables whose rows fit one 32-bit key
// space (table base + row) and whose entries fit 32-bit positions; per group, whatever the number
// of tables:
//   1. sa_prep_kernel      ids -> keys (out-of-range: the sentinel key, flagged) and positions
//   2. rocprim::radix_sort_pairs over the bits the key space needs (stable: equal keys keep list order)
//   3. sa_partial_kernel   a run longer than a 256-position chunk (the padding id of a history list
//                          owns most of B x T positions) is pre-summed per chunk by a whole
//                          workgroup, in a fixed order, into the workspace
//   4. sa_update_kernel    16 lanes per sorted position: a run head sums its entries (and the chunk
//                          partials behind it) and applies the row update; runs of more than
//                          kSaBig items are summed by the 16 lane groups of the workgroup together
// Tables flagged `coalesced` (sorted unique ids) form groups of their own that skip 2 and 3.
// No float atomics anywhere: every sum has a fixed order, so equal inputs give equal bits.
//
// The row update is a request-rate problem (every random row of p, m and v is one 128-B request,
// DESIGN.md section 5): a wave keeps four rows in flight (16 lanes x up to 4 columns each), the
// loads of p / m / v are issued before the gradient sum they do not depend on, and the kernel's
// register use leaves the full 8 waves per SIMD.
#include <rocprim/device/device_radix_sort.hpp>

#include <cmath>
#include <vector>

#include "common.h"

namespace rk {

constexpr int kSaMaxTables = 64;
constexpr int kSaChunk = 256;  // sorted positions per pre-summed chunk
constexpr int kSaLanes = 16;   // lanes per row
constexpr int kSaCols = 4;     // columns per lane and pass (64 columns per pass)
constexpr int kSaPass = kSaLanes * kSaCols;
constexpr int kSaGroups = 16;  // lane groups per workgroup
constexpr int kSaPos = 64;     // sorted positions per workgroup of the update kernel
constexpr int kSaBig = 32;     // a run of more items is summed by the whole workgroup

struct SaIndex {  // prep kernel
  const int64_t* idx[kSaMaxTables];
  int64_t idx_stride[kSaMaxTables];
  uint32_t key_base[kSaMaxTables + 1];  // first key of table t; [nt] = the sentinel
  uint32_t pos_base[kSaMaxTables + 1];  // first entry of table t in the group's entry list
};

struct SaTables {  // partial and update kernels
  float* param[kSaMaxTables];
  float* m[kSaMaxTables];
  float* v[kSaMaxTables];
  const float* values[kSaMaxTables];
  uint32_t key_base[kSaMaxTables + 1];
  uint32_t pos_base[kSaMaxTables + 1];
  int32_t ld[kSaMaxTables], ld_values[kSaMaxTables], dim[kSaMaxTables];
};

// Largest t in [0, nt) with base[t] <= x (base ascending, base[0] = 0).
__device__ __forceinline__ int sa_table_of(const uint32_t* base, int nt, uint32_t x) {
  int lo = 0, hi = nt - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (base[mid] <= x) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void sa_prep_kernel(SaIndex T, int nt, uint32_t n, uint32_t* __restrict__ keys,
                                                      uint32_t* __restrict__ pos, uint32_t* flags) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= n) return;
  const int t = sa_table_of(T.pos_base, nt, e);
  const int64_t r = T.idx[t][(int64_t)(e - T.pos_base[t]) * T.idx_stride[t]];
  const int64_t rows = (int64_t)T.key_base[t + 1] - (int64_t)T.key_base[t];
  const bool ok = r >= 0 && r < rows;
  if (!ok) flag_oob(flags);
  keys[e] = ok ? T.key_base[t] + (uint32_t)r : T.key_base[nt];
  pos[e] = e;
}

// One run of equal keys as a list of items: its first `nd` sorted positions from `i` on (up to the
// end of i's chunk), then the chunk partials c1, c1 + 1, ... behind them.
struct SaRun {
  uint32_t i, nd, c1, n;  // n = items in all
  int t;
};

__device__ __forceinline__ const float* sa_item(const SaRun& r, uint32_t j, const uint32_t* __restrict__ pos,
                                                const float* values, uint32_t pos_base, int64_t ld_values,
                                                const float* __restrict__ partial, int64_t ldp) {
  if (j < r.nd) return values + (int64_t)(pos[r.i + j] - pos_base) * ld_values;
  return partial + (int64_t)(r.c1 + (j - r.nd)) * ldp;
}

// acc[k] += column (col0 + 16 k) of items first, first + step, ... of the run, in that order; four
// items' loads are in flight together.
__device__ __forceinline__ void sa_accumulate(const SaRun& r, uint32_t first, uint32_t step, int col0, int dim,
                                              const uint32_t* __restrict__ pos, const float* values,
                                              uint32_t pos_base, int64_t ld_values,
                                              const float* __restrict__ partial, int64_t ldp,
                                              float (&acc)[kSaCols]) {
  for (uint32_t j = first; j < r.n; j += 4 * step) {
    const float* row[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint32_t jj = j + u * step;
      row[u] = jj < r.n ? sa_item(r, jj, pos, values, pos_base, ld_values, partial, ldp) : nullptr;
    }
    float x[4][kSaCols];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int k = 0; k < kSaCols; ++k) {
        const int c = col0 + kSaLanes * k;
        x[u][k] = (row[u] && c < dim) ? row[u][c] : 0.f;
      }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int k = 0; k < kSaCols; ++k) acc[k] += x[u][k];
  }
}

__device__ __forceinline__ void sa_row_update(float g, float& p, float& m, float& v, float omb1, float omb2,
                                              float eps, float step_size) {
  m = m + omb1 * (g - m);
  v = v + omb2 * (g * g - v);
  p = p - step_size * (m / (sqrtf(v) + eps));
}

// Chunk c >= 1 whose first position continues the run of chunk c - 1: the sum of its leading
// positions with that key, partial[c, 0:dim].  16 lane groups take positions g, g + 16, ... and
// their sums are added in group order.
__global__ __launch_bounds__(256) void sa_partial_kernel(SaTables T, int nt, uint32_t n,
                                                         const uint32_t* __restrict__ keys,
                                                         const uint32_t* __restrict__ pos,
                                                         float* __restrict__ partial, int64_t ldp) {
  __shared__ float part[kSaGroups][kSaPass];
  const uint32_t c = blockIdx.x + 1;
  const uint32_t i0 = c * (uint32_t)kSaChunk;
  const uint32_t key = keys[i0];
  if (keys[i0 - 1] != key || key == T.key_base[nt]) return;  // same for the whole workgroup
  const uint32_t i = i0 + threadIdx.x;
  const uint32_t len = (uint32_t)__syncthreads_count(i < n && keys[i] == key);  // sorted: a prefix of the chunk
  const int t = sa_table_of(T.key_base, nt, key);
  const int dim = T.dim[t];
  const int g = threadIdx.x / kSaLanes, l = threadIdx.x % kSaLanes;
  SaRun r;
  r.i = i0, r.nd = len, r.c1 = 0, r.n = len, r.t = t;
  for (int col = 0; col < dim; col += kSaPass) {
    float acc[kSaCols] = {0.f, 0.f, 0.f, 0.f};
    sa_accumulate(r, g, kSaGroups, col + l, dim, pos, T.values[t], T.pos_base[t], T.ld_values[t], partial, ldp,
                  acc);
#pragma unroll
    for (int k = 0; k < kSaCols; ++k) part[g][l + kSaLanes * k] = acc[k];
    __syncthreads();
    if (threadIdx.x < kSaPass && col + (int)threadIdx.x < dim) {
      float s = 0.f;
#pragma unroll
      for (int gg = 0; gg < kSaGroups; ++gg) s += part[gg][threadIdx.x];
      partial[(int64_t)c * ldp + col + threadIdx.x] = s;
    }
    __syncthreads();
  }
}

// First position after `i` whose key differs from keys[i] (galloping, then bisection).
__device__ __forceinline__ uint32_t sa_run_end(const uint32_t* __restrict__ keys, uint32_t n, uint32_t i,
                                               uint32_t key) {
  uint32_t lo = i, step = 1;  // keys[lo] == key
  uint32_t hi = n;            // keys[hi] != key or hi == n
  while (true) {
    const uint64_t probe = (uint64_t)lo + step;
    if (probe >= n) break;
    if (keys[probe] != key) {
      hi = (uint32_t)probe;
      break;
    }
    lo = (uint32_t)probe;
    step *= 2;
  }
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (keys[mid] == key) lo = mid;
    else hi = mid;
  }
  return hi;
}

// UNIQUE: every position is a run of its own (coalesced tables: no sort, no partials).
template <bool UNIQUE>
__global__ __launch_bounds__(256) void sa_update_kernel(SaTables T, int nt, uint32_t n,
                                                        const uint32_t* __restrict__ keys,
                                                        const uint32_t* __restrict__ pos,
                                                        const float* __restrict__ partial, int64_t ldp, float omb1,
                                                        float omb2, float eps, float step_size,
                                                        const float* __restrict__ step_size_dev) {
  __shared__ float part[kSaGroups][kSaPass];
  __shared__ SaRun big[kSaPos];
  __shared__ uint32_t big_key[kSaPos];
  __shared__ int nbig;
  if (step_size_dev) step_size = *step_size_dev;
  if (threadIdx.x == 0) nbig = 0;
  __syncthreads();
  const int g = threadIdx.x / kSaLanes, l = threadIdx.x % kSaLanes;
  const uint32_t sentinel = T.key_base[nt];
  for (int rr = 0; rr < kSaPos / kSaGroups; ++rr) {
    const uint64_t i64 = (uint64_t)blockIdx.x * kSaPos + rr * kSaGroups + g;
    if (i64 >= n) break;
    const uint32_t i = (uint32_t)i64;
    const uint32_t key = keys[i];
    if (key == sentinel) continue;
    SaRun r;
    r.i = i, r.nd = 1, r.c1 = 0, r.n = 1;
    if (!UNIQUE) {
      if (i > 0 && keys[i - 1] == key) continue;  // not a run head
      const uint32_t e = sa_run_end(keys, n, i, key);
      const uint32_t chunk_end = (i / kSaChunk + 1) * (uint32_t)kSaChunk;  // n < 2^32 - 256 (host)
      const uint32_t e0 = e < chunk_end ? e : chunk_end;
      r.nd = e0 - i;
      r.c1 = i / kSaChunk + 1;
      r.n = r.nd + (e > chunk_end ? (e - 1) / kSaChunk - r.c1 + 1 : 0);
    }
    const int t = sa_table_of(T.key_base, nt, key);
    r.t = t;
    if (r.n > (uint32_t)kSaBig) {  // left to the whole workgroup below
      if (l == 0) {
        const int b = atomicAdd(&nbig, 1);
        big[b] = r;
        big_key[b] = key;
      }
      continue;
    }
    const int dim = T.dim[t];
    const int64_t off = (int64_t)(key - T.key_base[t]) * T.ld[t];
    float *pp = T.param[t] + off, *pm = T.m[t] + off, *pv = T.v[t] + off;
    for (int col = 0; col < dim; col += kSaPass) {
      float p[kSaCols], m[kSaCols], v[kSaCols];
#pragma unroll
      for (int k = 0; k < kSaCols; ++k) {  // issued ahead of the gradient sum
        const int c = col + l + kSaLanes * k;
        const bool on = c < dim;
        p[k] = on ? pp[c] : 0.f;
        m[k] = on ? pm[c] : 0.f;
        v[k] = on ? pv[c] : 0.f;
      }
      float acc[kSaCols] = {0.f, 0.f, 0.f, 0.f};
      sa_accumulate(r, 0, 1, col + l, dim, pos, T.values[t], T.pos_base[t], T.ld_values[t], partial, ldp, acc);
#pragma unroll
      for (int k = 0; k < kSaCols; ++k) {
        const int c = col + l + kSaLanes * k;
        if (c < dim) {
          sa_row_update(acc[k], p[k], m[k], v[k], omb1, omb2, eps, step_size);
          pp[c] = p[k];
          pm[c] = m[k];
          pv[c] = v[k];
        }
      }
    }
  }
  if (UNIQUE) return;
  __syncthreads();
  const int nb = nbig;
  for (int b = 0; b < nb; ++b) {
    const SaRun r = big[b];
    const int t = r.t;
    const int dim = T.dim[t];
    const int64_t off = (int64_t)(big_key[b] - T.key_base[t]) * T.ld[t];
    for (int col = 0; col < dim; col += kSaPass) {
      float acc[kSaCols] = {0.f, 0.f, 0.f, 0.f};
      sa_accumulate(r, g, kSaGroups, col + l, dim, pos, T.values[t], T.pos_base[t], T.ld_values[t], partial, ldp,
                    acc);
#pragma unroll
      for (int k = 0; k < kSaCols; ++k) part[g][l + kSaLanes * k] = acc[k];
      __syncthreads();
      const int c = col + (int)threadIdx.x;
      if (threadIdx.x < kSaPass && c < dim) {
        float p = T.param[t][off + c], m = T.m[t][off + c], v = T.v[t][off + c];
        float s = 0.f;
#pragma unroll
        for (int gg = 0; gg < kSaGroups; ++gg) s += part[gg][threadIdx.x];
        sa_row_update(s, p, m, v, omb1, omb2, eps, step_size);
        T.param[t][off + c] = p;
        T.m[t][off + c] = m;
        T.v[t][off + c] = v;
      }
      __syncthreads();
    }
  }
}

// The device step counter (a float, torch's capturable layout): incremented here, the step size
// formed from it in double as the host form does and rounded to float once.
__global__ void sa_step_kernel(float* step, double lr, double beta1, double beta2, float* step_size) {
  const float t = *step + 1.f;
  *step = t;
  const double bc1 = 1.0 - pow(beta1, (double)t), bc2 = 1.0 - pow(beta2, (double)t);
  *step_size = (float)(lr * sqrt(bc2) / bc1);
}

// Column blocks of row-major matrices into contiguous [rows, dim] buffers, blockIdx.y = block.
struct SaPackList {
  rk_pack_block b[kSaMaxTables];
};
__global__ __launch_bounds__(256) void sa_pack_kernel(SaPackList L) {
  const rk_pack_block& b = L.b[blockIdx.y];
  const int64_t total = b.rows * b.dim;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t r = e / b.dim;
    const int c = (int)(e - r * b.dim);
    const float x = b.src[r * b.ld_src + c];
    b.dst[e] = b.add ? x + b.add[r * b.ld_add + c] : x;
  }
}

// ---- host ----
static size_t sa_align(size_t v) { return (v + 255) & ~(size_t)255; }

struct SaGroupPlan {
  std::vector<int> tables;
  bool coalesced = false;
  uint64_t rows = 0, nnz = 0;
  int maxdim = 0;
};

constexpr uint64_t kSaMaxRows = 0xFFFFFFFFull;               // keys 0 .. rows, the sentinel included
constexpr uint64_t kSaMaxNnz = 0xFFFFFFFFull - 2 * kSaChunk;  // 32-bit positions, chunk ends included

static int sa_plan(const rk_sparse_adam_tensor* ts, int32_t n, std::vector<SaGroupPlan>& groups, const char* who) {
  if (!ts || n < 0) return fail(RK_ERR_INVALID, "%s: bad arguments", who);
  int open[2] = {-1, -1};  // the group still taking tables: [0] sorted, [1] coalesced
  for (int i = 0; i < n; ++i) {
    const rk_sparse_adam_tensor& t = ts[i];
    if (t.rows <= 0 || t.dim <= 0 || t.ld < t.dim || t.ld > INT32_MAX || t.nnz < 0)
      return fail(RK_ERR_INVALID, "%s: tensor %d: bad rows / dim / ld / nnz", who, i);
    if ((uint64_t)t.rows > kSaMaxRows)
      return fail(RK_ERR_UNSUPPORTED, "%s: tensor %d: %lld rows do not fit 32-bit keys", who, i, (long long)t.rows);
    if ((uint64_t)t.nnz > kSaMaxNnz)
      return fail(RK_ERR_UNSUPPORTED, "%s: tensor %d: nnz %lld too large", who, i, (long long)t.nnz);
    if (t.nnz == 0) continue;
    if (!t.param || !t.exp_avg || !t.exp_avg_sq || !t.idx || !t.values || t.idx_stride < 1 || t.ld_values < t.dim ||
        t.ld_values > INT32_MAX)
      return fail(RK_ERR_INVALID, "%s: tensor %d: null pointer or bad stride", who, i);
    const int kind = t.coalesced ? 1 : 0;
    int gi = open[kind];
    if (gi < 0 || (int)groups[gi].tables.size() == kSaMaxTables || groups[gi].rows + (uint64_t)t.rows > kSaMaxRows ||
        groups[gi].nnz + (uint64_t)t.nnz > kSaMaxNnz) {
      groups.emplace_back();
      gi = open[kind] = (int)groups.size() - 1;
      groups[gi].coalesced = kind == 1;
    }
    SaGroupPlan& g = groups[gi];
    g.tables.push_back(i);
    g.rows += (uint64_t)t.rows;
    g.nnz += (uint64_t)t.nnz;
    g.maxdim = std::max(g.maxdim, (int)t.dim);
  }
  return RK_OK;
}

struct SaLayout {
  size_t sort_bytes = 0, off_k0 = 0, off_p0 = 0, off_k1 = 0, off_p1 = 0, off_partial = 0, off_tmp = 0, total = 0;
  int64_t ldp = 0;
};

// Workspace of one group behind the step-size slot; groups run one after another in the same bytes.
static SaLayout sa_layout(const SaGroupPlan& g) {
  SaLayout L;
  const size_t a = sa_align((size_t)g.nnz * sizeof(uint32_t));
  L.off_k0 = 256;
  L.off_p0 = L.off_k0 + a;
  L.total = L.off_p0 + a;
  if (g.coalesced) return L;
  (void)rocprim::radix_sort_pairs(nullptr, L.sort_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                  (uint32_t*)nullptr, (unsigned)g.nnz);
  L.off_k1 = L.total;
  L.off_p1 = L.off_k1 + a;
  L.off_partial = L.off_p1 + a;
  L.ldp = g.maxdim;
  const size_t chunks = ((size_t)g.nnz + kSaChunk - 1) / kSaChunk;
  L.off_tmp = L.off_partial + sa_align(chunks * (size_t)L.ldp * sizeof(float));
  L.total = L.off_tmp + sa_align(L.sort_bytes);
  return L;
}

}  // namespace rk

using namespace rk;

RK_API int rk_sparse_adam_step_workspace_size(const rk_sparse_adam_tensor* tensors, int32_t n, int64_t* bytes) {
  std::vector<SaGroupPlan> groups;
  if (!bytes) return fail(RK_ERR_INVALID, "rk_sparse_adam_step_workspace_size: bad arguments");
  const int rc = sa_plan(tensors, n, groups, "rk_sparse_adam_step_workspace_size");
  if (rc != RK_OK) return rc;
  size_t total = 256;
  for (const SaGroupPlan& g : groups) total = std::max(total, sa_layout(g).total);
  *bytes = (int64_t)total;
  return RK_OK;
}

RK_API int rk_sparse_adam_step(const rk_sparse_adam_tensor* tensors, int32_t n, double lr, double beta1, double beta2,
                               double eps, int64_t step, float* device_step, void* workspace, int64_t ws_bytes,
                               void* stream) {
  if ((step < 1 && !device_step) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !workspace)
    return fail(RK_ERR_INVALID, "rk_sparse_adam_step: bad arguments");
  std::vector<SaGroupPlan> groups;
  const int rc = sa_plan(tensors, n, groups, "rk_sparse_adam_step");
  if (rc != RK_OK) return rc;
  std::vector<SaLayout> layouts;  // one rocprim size query per group and call
  size_t need = 256;
  for (const SaGroupPlan& g : groups) {
    layouts.push_back(sa_layout(g));
    need = std::max(need, layouts.back().total);
  }
  if (ws_bytes < (int64_t)need)
    return fail(RK_ERR_INVALID, "rk_sparse_adam_step: workspace %lld < %zu bytes", (long long)ws_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  // scalars derived in double and rounded to float once, as rk_adam_step does
  const float omb1 = (float)(1.0 - beta1), omb2 = (float)(1.0 - beta2);
  float step_size = 0.f;
  float* step_size_dev = nullptr;
  if (device_step) {
    step_size_dev = reinterpret_cast<float*>(ws);
    sa_step_kernel<<<1, 1, 0, st>>>(device_step, lr, beta1, beta2, step_size_dev);
  } else {
    const double bc1 = 1.0 - std::pow(beta1, (double)step), bc2 = 1.0 - std::pow(beta2, (double)step);
    step_size = (float)(lr * std::sqrt(bc2) / bc1);
  }
  for (size_t gi = 0; gi < groups.size(); ++gi) {
    const SaGroupPlan& g = groups[gi];
    const SaLayout& L = layouts[gi];
    SaIndex I;
    SaTables T;
    const int nt = (int)g.tables.size();
    uint64_t kb = 0, pb = 0;
    for (int k = 0; k < nt; ++k) {
      const rk_sparse_adam_tensor& t = tensors[g.tables[k]];
      I.idx[k] = t.idx;
      I.idx_stride[k] = t.idx_stride;
      I.key_base[k] = T.key_base[k] = (uint32_t)kb;
      I.pos_base[k] = T.pos_base[k] = (uint32_t)pb;
      T.param[k] = t.param, T.m[k] = t.exp_avg, T.v[k] = t.exp_avg_sq, T.values[k] = t.values;
      T.ld[k] = (int32_t)t.ld, T.ld_values[k] = (int32_t)t.ld_values, T.dim[k] = t.dim;
      kb += (uint64_t)t.rows;
      pb += (uint64_t)t.nnz;
    }
    for (int k = nt; k <= kSaMaxTables; ++k) {
      I.key_base[k] = T.key_base[k] = (uint32_t)kb;
      I.pos_base[k] = T.pos_base[k] = (uint32_t)pb;
    }
    const uint32_t nn = (uint32_t)g.nnz;
    uint32_t *k0 = (uint32_t*)(ws + L.off_k0), *p0 = (uint32_t*)(ws + L.off_p0);
    sa_prep_kernel<<<(nn + 255) / 256, 256, 0, st>>>(I, nt, nn, k0, p0, device_flags());
    const unsigned blocks = (unsigned)(((uint64_t)nn + kSaPos - 1) / kSaPos);
    if (g.coalesced) {
      sa_update_kernel<true><<<blocks, 256, 0, st>>>(T, nt, nn, k0, p0, nullptr, 0, omb1, omb2, (float)eps,
                                                     step_size, step_size_dev);
      continue;
    }
    uint32_t *k1 = (uint32_t*)(ws + L.off_k1), *p1 = (uint32_t*)(ws + L.off_p1);
    float* partial = (float*)(ws + L.off_partial);
    int bits = 1;  // keys lie in [0, rows of the group]
    while (bits < 32 && ((uint64_t)1 << bits) <= g.rows) ++bits;
    size_t tb = L.sort_bytes;
    if (rocprim::radix_sort_pairs(ws + L.off_tmp, tb, k0, k1, p0, p1, nn, 0, bits, st) != hipSuccess)
      return fail(RK_ERR_LAUNCH, "rk_sparse_adam_step: radix sort failed");
    const unsigned chunks = (unsigned)(((uint64_t)nn + kSaChunk - 1) / kSaChunk);
    if (chunks > 1) sa_partial_kernel<<<chunks - 1, 256, 0, st>>>(T, nt, nn, k1, p1, partial, L.ldp);
    sa_update_kernel<false><<<blocks, 256, 0, st>>>(T, nt, nn, k1, p1, partial, L.ldp, omb1, omb2, (float)eps,
                                                    step_size, step_size_dev);
  }
  return check_launch("rk_sparse_adam_step");
}

RK_API int rk_pack_blocks(const rk_pack_block* blocks, int32_t n, void* stream) {
  if (!blocks || n < 0) return fail(RK_ERR_INVALID, "rk_pack_blocks: bad arguments");
  for (int base = 0; base < n; base += kSaMaxTables) {
    SaPackList L;
    const int cnt = std::min(kSaMaxTables, n - base);
    int64_t most = 0;
    for (int i = 0; i < cnt; ++i) {
      const rk_pack_block& b = blocks[base + i];
      if (b.rows < 0 || b.dim <= 0 || b.ld_src < b.dim || (b.rows > 0 && (!b.src || !b.dst)) ||
          (b.add && b.ld_add < b.dim))
        return fail(RK_ERR_INVALID, "rk_pack_blocks: block %d invalid", base + i);
      L.b[i] = b;
      most = std::max(most, b.rows * b.dim);
    }
    if (most == 0) continue;
    const unsigned gx = (unsigned)std::min<int64_t>((most + 255) / 256, 1024);
    sa_pack_kernel<<<dim3(gx, (unsigned)cnt), 256, 0, (hipStream_t)stream>>>(L);
  }
  return check_launch("rk_pack_blocks");
}
