// Per-request ranking on the device: the best k candidates of each request, and the AUC of each
// group (user) with its impression-weighted mean, GAUC.  Both are segmented operations over
// (score, group) on the flat [B] column that DIEN.score returns.
//
// Top-K order (both forms): score descending, -0.0 == +0.0, NaN below every number, ties by the
// lower row.  One 64-bit key holds it: (rank_bits(score) << 32) | (0xFFFFFFFF - row), larger is
// better; rank_bits is the usual order-preserving map of the float bits with -0.0 folded into +0.0
// and every NaN mapped to 0, below -inf's 0x007FFFFF.  Rows are < 2^32 - 1, so a real candidate's
// key is never 0 and 0 marks an empty slot.
//
// rk_topk_segments (contiguous candidates, k <= 64): one wave per request.  Lane l holds the l-th
// best key so far.  For each chunk of 64 new rows the wave first asks whether any new key beats the
// current k-th key (one ballot; if not, the chunk is done: with a running threshold most of a long
// segment is only read, four chunks' loads in flight at a time); otherwise it ranks the 128 keys by
// counting, each lane comparing its two keys with all 128 read lane by lane into scalar registers,
// and the keys of rank < k are scattered to their rank through 64 LDS slots.  Scores are read once;
// nothing is sorted globally.  A request is one wave's serial work, so very long segments belong to
// the sort path (rankops.ranking routes by n / R; DESIGN.md §4b has the measured crossover).
//
// rk_topk_by_request / rk_topk_segments_sorted (any order, any k <= 1024): a stable rocPRIM radix
// sort of (request << 32 | ~rank_bits) with the row as value over the 32 + bits(R) bits in use; a
// block per request then finds the request's range by binary search and writes its first k rows.
// Rows left out (bad request_index, no segment) sort under request R, past every real one.  The two
// forms order by the same (rank_bits, row) pair, so they agree bit for bit.
//
// rk_grouped_auc: rk_auc's integer scheme (metrics.hip) with the group in the high half of the sort
// key.  Sort (group, ascending score bits) with the label as value; reduce equal keys to (pos, neg);
// negatives-before by an exclusive scan that restarts at each group; reduce by group to
// (2U, P, N, has-NaN); one block writes the table and sums n_g * 2U_g / (2 P_g N_g) in a fixed order
// (strided per-thread sums, then a fixed tree), so the bits do not depend on the input row order.
// Counts that only the device knows (distinct keys, groups) stay there: the primitives run over n
// items and the iterators return neutral elements past the count, as rk_auc does.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce_by_key.hpp>
#include <rocprim/device/device_scan_by_key.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "common.h"

namespace rk {
namespace ranking {

typedef unsigned long long u64;

constexpr uint32_t kNoGroup = 0x80000000u;    // group of a row that is left out (valid ids are < 2^31)
constexpr uint32_t kPastCount = 0xFFFFFFFFu;  // group the iterators return past the device-side count
constexpr uint32_t kNanBits = 0xFFFFFFFFu;    // ascending score bits of every NaN

// Larger = ranks higher.  NaN -> 0, -inf -> 0x007FFFFF, -0.0 == +0.0 -> 0x80000000, +inf -> 0xFF800000.
__device__ __forceinline__ uint32_t rank_bits(float s) {
  uint32_t b = __float_as_uint(s);
  if (s != s) return 0u;
  if (b == 0x80000000u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// Ascending score bits for the AUC sort: the same map, except that every NaN becomes the largest key
// of its group, where the group reduction sees it.
__device__ __forceinline__ uint32_t auc_bits(float s) { return s != s ? kNanBits : rank_bits(s); }

__device__ __forceinline__ u64 readlane64(u64 v, int lane) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
  return ((u64)hi << 32) | lo;
}

__device__ __forceinline__ int64_t clamp_offset(int64_t o, int64_t n) { return o < 0 ? 0 : (o > n ? n : o); }

// ---------------- top-K, contiguous segments, k <= 64: one wave per request ----------------
constexpr int kChunksAhead = 4;

__global__ __launch_bounds__(64) void topk_segment_kernel(const float* __restrict__ scores, int64_t n,
                                                          const int64_t* __restrict__ offsets, int64_t R, int k,
                                                          float* __restrict__ values, int64_t* __restrict__ indices,
                                                          int64_t* __restrict__ counts, uint32_t* flags) {
  __shared__ u64 slot[64];
  const int lane = threadIdx.x;
  for (int64_t r = blockIdx.x; r < R; r += gridDim.x) {
    const int64_t o0 = offsets[r], o1 = offsets[r + 1];
    const int64_t lo = clamp_offset(o0, n);
    const int64_t hi = std::max(lo, clamp_offset(o1, n));
    if (lane == 0 && (lo != o0 || clamp_offset(o1, n) != o1)) flag_oob(flags);
    u64 best = 0;    // lane l: the l-th best key so far, 0 = none
    u64 thresh = 0;  // the k-th best key so far: a new key at or below it cannot enter
    for (int64_t base = lo; base < hi; base += 64 * kChunksAhead) {
      float sc[kChunksAhead];  // the loads of several chunks in flight before the first is looked at
#pragma unroll
      for (int u = 0; u < kChunksAhead; ++u) {
        const int64_t i = base + u * 64 + lane;
        sc[u] = i < hi ? scores[i] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < kChunksAhead; ++u) {
        const int64_t i = base + u * 64 + lane;
        u64 cand = 0;
        if (i < hi) cand = ((u64)rank_bits(sc[u]) << 32) | (u64)(0xFFFFFFFFu - (uint32_t)i);
        if (cand <= thresh) cand = 0;
        if (__ballot(cand != 0) == 0) continue;  // wave-uniform
        // rank of each lane's two keys among the 128 = the number of keys above it (non-zero keys are distinct)
        int rb = 0, rc = 0;
#pragma unroll
        for (int j = 0; j < 64; ++j) {
          const u64 bj = readlane64(best, j), cj = readlane64(cand, j);
          rb += (int)(bj > best) + (int)(cj > best);
          rc += (int)(bj > cand) + (int)(cj > cand);
        }
        slot[lane] = 0;
        __syncthreads();
        if (best != 0 && rb < k) slot[rb] = best;
        if (cand != 0 && rc < k) slot[rc] = cand;
        __syncthreads();
        best = slot[lane];
        __syncthreads();
        thresh = readlane64(best, k - 1);
      }
    }
    if (lane < k) {
      const int64_t o = r * k + lane;
      if (best != 0) {
        const uint32_t row = 0xFFFFFFFFu - (uint32_t)best;
        values[o] = scores[row];
        indices[o] = (int64_t)row;
      } else {
        values[o] = -INFINITY;
        indices[o] = -1;
      }
    }
    if (lane == 0) counts[r] = std::min<int64_t>(k, hi - lo);
  }
}

// ---------------- top-K, sort path ----------------
__global__ void topk_keys_by_request_kernel(const float* __restrict__ scores, const int64_t* __restrict__ req,
                                            int64_t n, int64_t R, u64* __restrict__ keys, uint32_t* __restrict__ rows,
                                            uint32_t* flags) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t r = req[i];
    if (r < 0 || r >= R) {
      flag_oob(flags);
      r = R;
    }
    keys[i] = ((u64)r << 32) | (u64)(uint32_t)~rank_bits(scores[i]);
    rows[i] = (uint32_t)i;
  }
}

__global__ void topk_keys_by_segment_kernel(const float* __restrict__ scores, const int64_t* __restrict__ offsets,
                                            int64_t n, int64_t R, u64* __restrict__ keys, uint32_t* __restrict__ rows,
                                            uint32_t* flags) {
  const int64_t first = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = first; i <= R; i += step)
    if (offsets[i] < 0 || offsets[i] > n) flag_oob(flags);
  for (int64_t i = first; i < n; i += step) {
    // the number of offsets[0..R] at or below i; the segment is the last of them
    int64_t lo = 0, hi = R + 1;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (clamp_offset(offsets[mid], n) <= i) lo = mid + 1;
      else hi = mid;
    }
    const int64_t r = (lo >= 1 && lo <= R) ? lo - 1 : R;
    keys[i] = ((u64)r << 32) | (u64)(uint32_t)~rank_bits(scores[i]);
    rows[i] = (uint32_t)i;
  }
}

// first index in keys[0..n) whose key is >= v
__device__ __forceinline__ int64_t lower_bound_u64(const u64* __restrict__ keys, int64_t n, u64 v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(64) void topk_write_sorted_kernel(const float* __restrict__ scores,
                                                               const u64* __restrict__ keys,
                                                               const uint32_t* __restrict__ rows, int64_t n, int64_t R,
                                                               int k, float* __restrict__ values,
                                                               int64_t* __restrict__ indices,
                                                               int64_t* __restrict__ counts) {
  for (int64_t r = blockIdx.x; r < R; r += gridDim.x) {
    const int64_t s = lower_bound_u64(keys, n, (u64)r << 32);
    const int64_t e = lower_bound_u64(keys, n, (u64)(r + 1) << 32);
    const int64_t cnt = e - s;
    for (int j = threadIdx.x; j < k; j += 64) {
      const int64_t o = r * k + j;
      if (j < cnt) {
        const uint32_t row = rows[s + j];
        values[o] = scores[row];
        indices[o] = (int64_t)row;
      } else {
        values[o] = -INFINITY;
        indices[o] = -1;
      }
    }
    if (threadIdx.x == 0) counts[r] = std::min<int64_t>(k, cnt);
  }
}

struct TopkPlan {
  size_t sort_bytes, total;
  size_t off_keys_in, off_keys_out, off_rows_in, off_rows_out, off_tmp;
  unsigned end_bit;
};

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

static TopkPlan topk_plan(int64_t n, int64_t R) {
  TopkPlan p{};
  unsigned bits = 0;
  while (((int64_t)1 << bits) <= R) ++bits;  // request R (rows left out) included
  p.end_bit = 32 + bits;
  const int64_t m = std::max<int64_t>(n, 1);
  u64* k = nullptr;
  uint32_t* v = nullptr;
  (void)rocprim::radix_sort_pairs(nullptr, p.sort_bytes, k, k, v, v, (unsigned)m, 0, p.end_bit);
  size_t o = 0;
  p.off_keys_in = o;
  o += align256(m * sizeof(u64));
  p.off_keys_out = o;
  o += align256(m * sizeof(u64));
  p.off_rows_in = o;
  o += align256(m * sizeof(uint32_t));
  p.off_rows_out = o;
  o += align256(m * sizeof(uint32_t));
  p.off_tmp = o;
  o += align256(p.sort_bytes);
  p.total = o;
  return p;
}

inline bool topk_sizes_ok(int64_t n, int64_t R, int32_t k) {
  return n >= 0 && n <= (int64_t)UINT32_MAX - 1 && R >= 0 && R <= (int64_t)INT32_MAX && k >= 1 && k <= RK_TOPK_MAX_K;
}

// The sort path behind both sorted entry points; exactly one of request_index / offsets is given.
static int topk_sorted(const char* what, const float* scores, const int64_t* request_index, const int64_t* offsets,
                       int64_t n, int64_t R, int32_t k, float* values, int64_t* indices, int64_t* counts,
                       void* workspace, int64_t ws_bytes, void* stream) {
  if (!topk_sizes_ok(n, R, k) || (n > 0 && (!scores || !(request_index || offsets))) || !values || !indices ||
      !counts || !workspace)
    return fail(RK_ERR_INVALID, "%s: bad arguments (n=%lld, R=%lld, k=%d)", what, (long long)n, (long long)R, k);
  const TopkPlan p = topk_plan(n, R);
  if (ws_bytes < (int64_t)p.total)
    return fail(RK_ERR_INVALID, "%s: workspace %lld < %zu bytes", what, (long long)ws_bytes, p.total);
  if (R == 0) return RK_OK;
  hipStream_t st = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  u64* keys_in = reinterpret_cast<u64*>(ws + p.off_keys_in);
  u64* keys_out = reinterpret_cast<u64*>(ws + p.off_keys_out);
  uint32_t* rows_in = reinterpret_cast<uint32_t*>(ws + p.off_rows_in);
  uint32_t* rows_out = reinterpret_cast<uint32_t*>(ws + p.off_rows_out);
  if (n > 0) {
    const int64_t work = request_index ? n : std::max(n, R + 1);
    const unsigned blocks = (unsigned)std::min<int64_t>((work + 255) / 256, 8 * (int64_t)num_cus());
    if (request_index)
      topk_keys_by_request_kernel<<<blocks, 256, 0, st>>>(scores, request_index, n, R, keys_in, rows_in,
                                                          device_flags());
    else
      topk_keys_by_segment_kernel<<<blocks, 256, 0, st>>>(scores, offsets, n, R, keys_in, rows_in, device_flags());
    size_t b = p.sort_bytes;
    if (rocprim::radix_sort_pairs(ws + p.off_tmp, b, keys_in, keys_out, rows_in, rows_out, (unsigned)n, 0, p.end_bit,
                                  st) != hipSuccess)
      return fail(RK_ERR_RUNTIME, "%s: radix sort failed", what);
  }
  const unsigned blocks = (unsigned)std::min<int64_t>(R, 64 * (int64_t)num_cus());
  topk_write_sorted_kernel<<<blocks, 64, 0, st>>>(scores, keys_out, rows_out, n, R, k, values, indices, counts);
  return check_launch(what);
}

// ---------------- grouped AUC ----------------
struct PN {
  long long pos, neg;
};
struct LabelPN {
  __host__ __device__ PN operator()(float y) const { return y > 0.5f ? PN{1, 0} : PN{0, 1}; }
};
struct PlusPNs {
  __host__ __device__ PN operator()(const PN& a, const PN& b) const { return {a.pos + b.pos, a.neg + b.neg}; }
};
struct GStat {
  long long two_u, pos, neg, nan;
};
struct PlusGStat {
  __host__ __device__ GStat operator()(const GStat& a, const GStat& b) const {
    return {a.two_u + b.two_u, a.pos + b.pos, a.neg + b.neg, a.nan + b.nan};
  }
};
// Over the distinct (group, score) keys i = 0 .. *cnt - 1; past the count: a group of its own, zeros.
struct KeyGroup {
  const u64* ukeys;
  const unsigned* cnt;
  __host__ __device__ uint32_t operator()(unsigned i) const {
    return i < *cnt ? (uint32_t)(ukeys[i] >> 32) : kPastCount;
  }
};
struct KeyNeg {
  const PN* agg;
  const unsigned* cnt;
  __host__ __device__ long long operator()(unsigned i) const { return i < *cnt ? agg[i].neg : 0ll; }
};
struct KeyStat {
  const PN* agg;
  const long long* neg_before;
  const u64* ukeys;
  const unsigned* cnt;
  __host__ __device__ GStat operator()(unsigned i) const {
    if (i >= *cnt) return {0, 0, 0, 0};
    const PN a = agg[i];
    return {a.pos * (2 * neg_before[i] + a.neg), a.pos, a.neg, (uint32_t)ukeys[i] == kNanBits ? 1ll : 0ll};
  }
};

__global__ void gauc_keys_kernel(const float* __restrict__ scores, const int64_t* __restrict__ groups, int64_t n,
                                 u64* __restrict__ keys, uint32_t* flags) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t g = groups[i];
    uint32_t gid = (uint32_t)g;
    if (g < 0 || g >= (int64_t)kNoGroup) {
      flag_oob(flags);
      gid = kNoGroup;
    }
    keys[i] = ((u64)gid << 32) | (u64)auc_bits(scores[i]);
  }
}

constexpr int kFinalThreads = 1024;

// One block: the table of the groups present (ascending id: the sort's order; the groups of rows
// left out and of the padding sort last) and the weighted mean, summed in a fixed order.
__global__ __launch_bounds__(kFinalThreads) void gauc_final_kernel(
    const uint32_t* __restrict__ gkeys, const GStat* __restrict__ gstat, const unsigned* __restrict__ gcnt,
    int64_t* __restrict__ ids, int64_t* __restrict__ two_u, int64_t* __restrict__ pos, int64_t* __restrict__ neg,
    int64_t* __restrict__ n_groups, void* summary) {
  __shared__ double s_num[kFinalThreads / 64];
  __shared__ long long s_cnt[4][kFinalThreads / 64];
  const unsigned G = *gcnt;
  double num = 0.0;
  long long present = 0, valid = 0, rows = 0, nan = 0;
  for (unsigned g = threadIdx.x; g < G; g += kFinalThreads) {
    const uint32_t id = gkeys[g];
    if (id >= kNoGroup) continue;
    const GStat s = gstat[g];
    ids[g] = (int64_t)id;
    two_u[g] = s.two_u;
    pos[g] = s.pos;
    neg[g] = s.neg;
    ++present;
    if (s.pos > 0 && s.neg > 0) {
      ++valid;
      rows += s.pos + s.neg;
      nan += s.nan;
      num += (double)(s.pos + s.neg) * ((double)s.two_u / (2.0 * (double)s.pos * (double)s.neg));
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    num += __shfl_down(num, o, kWave);
    present += __shfl_down(present, o, kWave);
    valid += __shfl_down(valid, o, kWave);
    rows += __shfl_down(rows, o, kWave);
    nan += __shfl_down(nan, o, kWave);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_num[w] = num;
    s_cnt[0][w] = present;
    s_cnt[1][w] = valid;
    s_cnt[2][w] = rows;
    s_cnt[3][w] = nan;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    long long c[4] = {0, 0, 0, 0};
    for (int i = 0; i < kFinalThreads / 64; ++i) {
      t += s_num[i];
      for (int q = 0; q < 4; ++q) c[q] += s_cnt[q][i];
    }
    *n_groups = c[0];
    double* gauc = static_cast<double*>(summary);
    long long* tail = reinterpret_cast<long long*>(gauc + 1);
    *gauc = (c[1] == 0 || c[3] != 0) ? __builtin_nan("") : t / (double)c[2];
    tail[0] = c[1];
    tail[1] = c[2];
  }
}

struct GaucPlan {
  size_t sort_bytes, rbk_bytes, scan_bytes, rbg_bytes, total;
  size_t off_keys_in, off_keys_out, off_vals, off_agg, off_cnt, off_nb, off_gkeys, off_gstat, off_gcnt, off_tmp;
};

static GaucPlan gauc_plan(int64_t n) {
  GaucPlan p{};
  const unsigned un = (unsigned)n;
  u64* k = nullptr;
  float* f = nullptr;
  (void)rocprim::radix_sort_pairs(nullptr, p.sort_bytes, k, k, f, f, un, 0, 64);
  (void)rocprim::reduce_by_key(nullptr, p.rbk_bytes, k, rocprim::make_transform_iterator(f, LabelPN()), un, k,
                               (PN*)nullptr, (unsigned*)nullptr, PlusPNs());
  rocprim::counting_iterator<unsigned> idx(0);
  auto kg = rocprim::make_transform_iterator(idx, KeyGroup{nullptr, nullptr});
  (void)rocprim::exclusive_scan_by_key(nullptr, p.scan_bytes, kg,
                                       rocprim::make_transform_iterator(idx, KeyNeg{nullptr, nullptr}),
                                       (long long*)nullptr, 0ll, (size_t)un, rocprim::plus<long long>());
  (void)rocprim::reduce_by_key(nullptr, p.rbg_bytes, kg,
                               rocprim::make_transform_iterator(idx, KeyStat{nullptr, nullptr, nullptr, nullptr}), un,
                               (uint32_t*)nullptr, (GStat*)nullptr, (unsigned*)nullptr, PlusGStat());
  size_t o = 0;
  p.off_keys_in = o;  // the keys as built; after the sort, the distinct keys
  o += align256(n * sizeof(u64));
  p.off_keys_out = o;
  o += align256(n * sizeof(u64));
  p.off_vals = o;
  o += align256(n * sizeof(float));
  p.off_agg = o;
  o += align256(n * sizeof(PN));
  p.off_cnt = o;
  o += align256(sizeof(unsigned));
  p.off_nb = o;
  o += align256(n * sizeof(long long));
  p.off_gkeys = o;
  o += align256(n * sizeof(uint32_t));
  p.off_gstat = o;
  o += align256(n * sizeof(GStat));
  p.off_gcnt = o;
  o += align256(sizeof(unsigned));
  p.off_tmp = o;
  o += align256(std::max(std::max(p.sort_bytes, p.rbk_bytes), std::max(p.scan_bytes, p.rbg_bytes)));
  p.total = o;
  return p;
}

}  // namespace ranking
}  // namespace rk

using namespace rk;
using namespace rk::ranking;

RK_API int rk_topk_segments(const float* scores, int64_t n, const int64_t* offsets, int64_t R, int32_t k,
                            float* values, int64_t* indices, int64_t* counts, void* stream) {
  if (!topk_sizes_ok(n, R, k) || (n > 0 && !scores) || !offsets || !values || !indices || !counts)
    return fail(RK_ERR_INVALID, "rk_topk_segments: bad arguments (n=%lld, R=%lld, k=%d)", (long long)n, (long long)R,
                k);
  if (k > RK_TOPK_SEGMENT_MAX_K)
    return fail(RK_ERR_UNSUPPORTED, "rk_topk_segments: k=%d > %d (use rk_topk_segments_sorted)", k,
                RK_TOPK_SEGMENT_MAX_K);
  if (R == 0) return RK_OK;
  const unsigned blocks = (unsigned)std::min<int64_t>(R, 64 * (int64_t)num_cus());
  topk_segment_kernel<<<blocks, 64, 0, (hipStream_t)stream>>>(scores, n, offsets, R, k, values, indices, counts,
                                                              device_flags());
  return check_launch("rk_topk_segments");
}

RK_API int rk_topk_by_request_workspace_size(int64_t n, int64_t R, int64_t* bytes) {
  if (!topk_sizes_ok(n, R, 1) || !bytes)
    return fail(RK_ERR_INVALID, "rk_topk_by_request_workspace_size: bad arguments (n=%lld, R=%lld)", (long long)n,
                (long long)R);
  *bytes = (int64_t)topk_plan(n, R).total;
  return RK_OK;
}

RK_API int rk_topk_segments_sorted(const float* scores, int64_t n, const int64_t* offsets, int64_t R, int32_t k,
                                   float* values, int64_t* indices, int64_t* counts, void* workspace,
                                   int64_t ws_bytes, void* stream) {
  if (!offsets) return fail(RK_ERR_INVALID, "rk_topk_segments_sorted: offsets is NULL");
  return topk_sorted("rk_topk_segments_sorted", scores, nullptr, offsets, n, R, k, values, indices, counts, workspace,
                     ws_bytes, stream);
}

RK_API int rk_topk_by_request(const float* scores, const int64_t* request_index, int64_t n, int64_t R, int32_t k,
                              float* values, int64_t* indices, int64_t* counts, void* workspace, int64_t ws_bytes,
                              void* stream) {
  if (n > 0 && !request_index) return fail(RK_ERR_INVALID, "rk_topk_by_request: request_index is NULL");
  return topk_sorted("rk_topk_by_request", scores, request_index, nullptr, n, R, k, values, indices, counts,
                     workspace, ws_bytes, stream);
}

RK_API int rk_grouped_auc_workspace_size(int64_t n, int64_t* bytes) {
  if (n < 0 || n > (int64_t)UINT32_MAX - 1 || !bytes)
    return fail(RK_ERR_INVALID, "rk_grouped_auc_workspace_size: bad n");
  *bytes = (int64_t)gauc_plan(std::max<int64_t>(n, 1)).total;
  return RK_OK;
}

RK_API int rk_grouped_auc(const float* scores, const float* labels, const int64_t* groups, int64_t n,
                          void* workspace, int64_t ws_bytes, void* summary, int64_t* group_ids, int64_t* two_u,
                          int64_t* pos, int64_t* neg, int64_t* n_groups, void* stream) {
  if (!scores || !labels || !groups || !workspace || !summary || !group_ids || !two_u || !pos || !neg || !n_groups ||
      n <= 0 || n > (int64_t)UINT32_MAX - 1)
    return fail(RK_ERR_INVALID, "rk_grouped_auc: bad arguments (n=%lld)", (long long)n);
  const GaucPlan p = gauc_plan(n);
  if (ws_bytes < (int64_t)p.total)
    return fail(RK_ERR_INVALID, "rk_grouped_auc: workspace %lld < %zu bytes", (long long)ws_bytes, p.total);
  hipStream_t st = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  u64* keys_in = reinterpret_cast<u64*>(ws + p.off_keys_in);
  u64* keys = reinterpret_cast<u64*>(ws + p.off_keys_out);
  float* vals = reinterpret_cast<float*>(ws + p.off_vals);
  u64* ukeys = keys_in;  // free again once the sort has read it
  PN* agg = reinterpret_cast<PN*>(ws + p.off_agg);
  unsigned* cnt = reinterpret_cast<unsigned*>(ws + p.off_cnt);
  long long* nb = reinterpret_cast<long long*>(ws + p.off_nb);
  uint32_t* gkeys = reinterpret_cast<uint32_t*>(ws + p.off_gkeys);
  GStat* gstat = reinterpret_cast<GStat*>(ws + p.off_gstat);
  unsigned* gcnt = reinterpret_cast<unsigned*>(ws + p.off_gcnt);
  void* tmp = ws + p.off_tmp;
  const unsigned un = (unsigned)n;
  const unsigned blocks = (unsigned)std::min<int64_t>((n + 255) / 256, 8 * (int64_t)num_cus());
  gauc_keys_kernel<<<blocks, 256, 0, st>>>(scores, groups, n, keys_in, device_flags());
  size_t b = p.sort_bytes;
  if (rocprim::radix_sort_pairs(tmp, b, keys_in, keys, labels, vals, un, 0, 64, st) != hipSuccess)
    return fail(RK_ERR_RUNTIME, "rk_grouped_auc: radix sort failed");
  b = p.rbk_bytes;
  if (rocprim::reduce_by_key(tmp, b, keys, rocprim::make_transform_iterator(vals, LabelPN()), un, ukeys, agg, cnt,
                             PlusPNs(), rocprim::equal_to<u64>(), st) != hipSuccess)
    return fail(RK_ERR_RUNTIME, "rk_grouped_auc: reduce_by_key failed");
  rocprim::counting_iterator<unsigned> idx(0);
  auto kg = rocprim::make_transform_iterator(idx, KeyGroup{ukeys, cnt});
  b = p.scan_bytes;
  if (rocprim::exclusive_scan_by_key(tmp, b, kg, rocprim::make_transform_iterator(idx, KeyNeg{agg, cnt}), nb, 0ll,
                                     (size_t)un, rocprim::plus<long long>(), rocprim::equal_to<uint32_t>(),
                                     st) != hipSuccess)
    return fail(RK_ERR_RUNTIME, "rk_grouped_auc: scan_by_key failed");
  b = p.rbg_bytes;
  if (rocprim::reduce_by_key(tmp, b, kg, rocprim::make_transform_iterator(idx, KeyStat{agg, nb, ukeys, cnt}), un, gkeys,
                             gstat, gcnt, PlusGStat(), rocprim::equal_to<uint32_t>(), st) != hipSuccess)
    return fail(RK_ERR_RUNTIME, "rk_grouped_auc: group reduce_by_key failed");
  gauc_final_kernel<<<1, kFinalThreads, 0, st>>>(gkeys, gstat, gcnt, group_ids, two_u, pos, neg, n_groups, summary);
  return check_launch("rk_grouped_auc");
}
