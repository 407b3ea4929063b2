// Weight-gradient GEMM of the training backward: dW[n][k] = sum_r dZ[r][n] X[r][k]
// and the bias gradient db[n] = sum_r dZ[r][n] over a long reduction (r = batch rows, 131,072 for
// BST's per-position projections), the `loss.backward()` of every nn.Linear in the reference's
// train() loops (bst.py:59-64,73-75,86-90; dcn.py:147-150; din.py:272-285).
//
// Shape: output N x K <= 128 x 128 per tile, reduction R >> N, K.  rk_gemm's 64 x 64 split-K tiles
// read every operand column block twice (once per output tile sharing it) and combine with float
// atomics; here one 512-thread workgroup owns a whole 128 x 128 output tile for a slab of rows, so
// dZ and X are each read once from HBM, and the slabs' partial tiles go to a workspace summed in a
// fixed order by a second kernel (deterministic).
//   * 64-row steps staged into a k-major (transposed) LDS image [128 cols][64 rows + 4] per operand:
//     float4 global loads, a 4 x 4 register transpose, ds_write_b128; the next step's loads are in
//     flight during this step's MFMAs;
//   * wave w owns n rows 32 (w & 3) .. +32 and k columns 64 (w >> 2) .. +64: two
//     v_mfma_f32_32x32x2_f32 tiles; each lane reads 4 consecutive reduction rows of its column with
//     one ds_read_b128 (3 reads per 8 MFMAs; the row-major image needed 8, and measured 51 us);
//   * the bias sums come from the staged registers (each thread's four columns, all its rows) and
//     are folded across the workgroup once at the end.
#include "common.h"

namespace rk {

constexpr int kWgT = 128;        // output tile edge (n and k)
constexpr int kWgR = 64;         // rows per step
constexpr int kWgP = kWgR + 4;   // LDS pitch of the k-major image S[col][row] (floats)
constexpr int kWgThreads = 512;
static_assert(kWgR * kWgT == 16 * kWgThreads, "one 4 x 4 staging block per thread and operand");

// Staging: thread t owns the 4 x 4 block (rows 4 (t >> 5) .. +3 of the step, columns 4 (t & 31) .. +3)
// of each operand: four float4 row loads (a wave covers two rows x 512 B per instruction), then a
// register transpose and four ds_write_b128 into the k-major LDS image S[col][row] (pitch kWgP), so
// the MFMA loop reads 4 consecutive reduction rows per lane with one ds_read_b128.
// Raw loads only (out-of-range rows / columns read a clamped in-range address): the zeroing and
// masking happen in wg_store, so nothing consumes the loaded registers until the next step's store
// and the loads stay in flight across this step's MFMAs.
template <bool MASK>
__device__ __forceinline__ void wg_load(const float* __restrict__ P, int64_t ld, const float* __restrict__ mask,
                                        int64_t r0, int64_t re, int c0, int cols, int tid, f32x4 (&v)[4],
                                        f32x4 (&m)[4]) {
  const int c = 4 * (tid & 31);
  const int cc = c0 + c < cols ? c0 + c : c0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t r = min<int64_t>(r0 + 4 * (tid >> 5) + i, re - 1);
    v[i] = *reinterpret_cast<const f32x4*>(P + r * ld + cc);
    if (MASK) m[i] = *reinterpret_cast<const f32x4*>(mask + r * ld + cc);
  }
}

// Store a staged step (rows >= re / columns >= cols zeroed, mask applied) transposed into the
// k-major LDS image; adds the stored values to bsum (per column) when SUMS.
template <bool MASK, bool SUMS>
__device__ __forceinline__ void wg_store(float* __restrict__ S, int tid, const f32x4 (&v)[4], const f32x4 (&m)[4],
                                         int64_t r0, int64_t re, int c0, int cols, f32x4& bsum) {
  const bool cok = c0 + 4 * (tid & 31) < cols;
  f32x4 x[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const bool ok = cok && r0 + 4 * (tid >> 5) + i < re;
#pragma unroll
    for (int e = 0; e < 4; ++e) x[i][e] = (ok && (!MASK || m[i][e] > 0.f)) ? v[i][e] : 0.f;
    if (SUMS) bsum += x[i];
  }
#pragma unroll
  for (int e = 0; e < 4; ++e)
    *reinterpret_cast<f32x4*>(S + (4 * (tid & 31) + e) * kWgP + 4 * (tid >> 5)) =
        f32x4{x[0][e], x[1][e], x[2][e], x[3][e]};
}

// grid (splits, n tiles, k tiles); partial tile of split s -> ws[s][n][k] (N x K), bias partial ->
// wsb[s][n].
template <bool MASK>
__global__ __launch_bounds__(kWgThreads) void wgrad_kernel(int64_t N, int64_t K, int64_t R, int64_t rps,
                                                           const float* __restrict__ A, int64_t lda,
                                                           const float* __restrict__ A_mask,
                                                           const float* __restrict__ B, int64_t ldb,
                                                           float* __restrict__ ws, float* __restrict__ wsb) {
#define RK_WG_TILE_N blockIdx.y
#define RK_WG_TILE_K blockIdx.z
#include "wgrad_tile.h"
#undef RK_WG_TILE_N
#undef RK_WG_TILE_K
}

// G problems of one shape in one launch (rk_gemm_wgrad_grouped): grid (splits, n tiles x k tiles, G);
// group g's operands by pointer, its partials in its own stretch of the workspace.
constexpr int kWgMaxGroups = 16;
struct WgradGroups {
  const float* A[kWgMaxGroups];
  const float* B[kWgMaxGroups];
  float* C[kWgMaxGroups];
  float* row_sums[kWgMaxGroups];
};

__global__ __launch_bounds__(kWgThreads) void wgrad_grouped_kernel(WgradGroups gp, int64_t N, int64_t K, int64_t R,
                                                                   int64_t rps, int64_t lda, int64_t ldb,
                                                                   float* __restrict__ ws_all, int64_t ws_group,
                                                                   int64_t splits, int with_sums) {
  constexpr bool MASK = false;
  const int nt = (int)((N + kWgT - 1) / kWgT);
  const float* __restrict__ A = gp.A[blockIdx.z];
  const float* __restrict__ B = gp.B[blockIdx.z];
  const float* A_mask = nullptr;
  float* __restrict__ ws = ws_all + blockIdx.z * ws_group;
  float* __restrict__ wsb = with_sums ? ws + splits * N * K : nullptr;
#define RK_WG_TILE_N (blockIdx.y % nt)
#define RK_WG_TILE_K (blockIdx.y / nt)
#include "wgrad_tile.h"
#undef RK_WG_TILE_N
#undef RK_WG_TILE_K
}

// C[n][k] (+)= sum_s ws[s][n][k] (float4 per lane, the 16 waves of a workgroup split s, fixed-order
// LDS combine); the workgroups past the tile's float4 count do the same for row_sums from wsb.
__global__ __launch_bounds__(1024) void wgrad_reduce_kernel(const float* __restrict__ ws, const float* __restrict__ wsb,
                                                            int64_t S, int64_t N, int64_t K, float* __restrict__ C,
                                                            int64_t ldc, float* __restrict__ row_sums, int accumulate,
                                                            int64_t c_blocks) {
#include "wgrad_reduce.h"
}

// grid (c_blocks + bias blocks, G)
__global__ __launch_bounds__(1024) void wgrad_reduce_grouped_kernel(WgradGroups gp, const float* __restrict__ ws_all,
                                                                    int64_t ws_group, int64_t S, int64_t N, int64_t K,
                                                                    int64_t ldc, int accumulate, int64_t c_blocks) {
  const float* __restrict__ ws = ws_all + blockIdx.y * ws_group;
  const float* __restrict__ wsb = ws + S * N * K;
  float* __restrict__ C = gp.C[blockIdx.y];
  float* __restrict__ row_sums = gp.row_sums[blockIdx.y];
#include "wgrad_reduce.h"
}

static int64_t wgrad_splits(int64_t N, int64_t K, int64_t R, int64_t G = 1) {
  const int64_t tiles = G * ((N + kWgT - 1) / kWgT) * ((K + kWgT - 1) / kWgT);
  // one workgroup per CU and output tile.  Two per CU (4 waves / SIMD) measured no faster
  // (tools/wgrad_clock.cpp: 40.7 us for half the rows vs 42.9 us), and the partial tiles double.
  const int64_t want = std::max<int64_t>(1, num_cus() / tiles);
  const int64_t steps = (R + kWgR - 1) / kWgR;
  return std::max<int64_t>(1, std::min<int64_t>(want, steps));
}

}  // namespace rk

using namespace rk;

RK_API int64_t rk_gemm_wgrad_workspace_floats(int64_t N, int64_t K, int64_t R) {
  if (N <= 0 || K <= 0 || R < 0) return 0;
  return wgrad_splits(N, K, R) * (N * K + N);
}

RK_API int rk_gemm_wgrad(int64_t N, int64_t K, int64_t R, const float* A, int64_t lda, const float* A_mask,
                         const float* B, int64_t ldb, float* C, int64_t ldc, float* row_sums, int32_t accumulate,
                         float* workspace, int64_t workspace_floats, void* stream) {
  if (N <= 0 || K <= 0 || R < 0 || !C || ldc < K || (R > 0 && (!A || !B)) || lda < N || ldb < K)
    return fail(RK_ERR_INVALID, "rk_gemm_wgrad: bad shape / operand");
  const uintptr_t align = reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B) |
                          reinterpret_cast<uintptr_t>(A_mask) | reinterpret_cast<uintptr_t>(C) |
                          reinterpret_cast<uintptr_t>(row_sums) | reinterpret_cast<uintptr_t>(workspace);
  if ((N | K | lda | ldb | ldc) % 4 || (align & 15))
    return fail(RK_ERR_UNSUPPORTED, "rk_gemm_wgrad: needs N, K, lda, ldb, ldc multiples of 4 and 16-B aligned "
                                    "pointers (use rk_gemm)");
  if (!workspace || workspace_floats < rk_gemm_wgrad_workspace_floats(N, K, R))
    return fail(RK_ERR_INVALID, "rk_gemm_wgrad: workspace of %lld floats, needs %lld", (long long)workspace_floats,
                (long long)rk_gemm_wgrad_workspace_floats(N, K, R));
  hipStream_t st = (hipStream_t)stream;
  const int64_t S = wgrad_splits(N, K, R);
  int64_t rps = (R + S - 1) / S;
  rps = std::max<int64_t>(kWgR, (rps + kWgR - 1) / kWgR * kWgR);
  const int64_t splits = std::max<int64_t>(1, (R + rps - 1) / rps);
  float* wsb = workspace + splits * N * K;
  if (R > 0) {
    const dim3 grid((unsigned)splits, (unsigned)((N + kWgT - 1) / kWgT), (unsigned)((K + kWgT - 1) / kWgT));
    if (A_mask)
      wgrad_kernel<true><<<grid, kWgThreads, 0, st>>>(N, K, R, rps, A, lda, A_mask, B, ldb, workspace,
                                                      row_sums ? wsb : nullptr);
    else
      wgrad_kernel<false><<<grid, kWgThreads, 0, st>>>(N, K, R, rps, A, lda, nullptr, B, ldb, workspace,
                                                       row_sums ? wsb : nullptr);
  } else {
    (void)hipMemsetAsync(workspace, 0, sizeof(float) * (size_t)(N * K + N), st);
  }
  const int64_t c_blocks = (N * K / 4 + 63) / 64;
  const int64_t b_blocks = row_sums ? (N / 4 + 63) / 64 : 0;
  wgrad_reduce_kernel<<<(unsigned)(c_blocks + b_blocks), 1024, 0, st>>>(workspace, wsb, R > 0 ? splits : 1, N, K, C,
                                                                       ldc, row_sums, accumulate, c_blocks);
  return check_launch("rk_gemm_wgrad");
}

RK_API int64_t rk_gemm_wgrad_grouped_workspace_floats(int32_t G, int64_t N, int64_t K, int64_t R) {
  if (G <= 0 || N <= 0 || K <= 0 || R < 0) return 0;
  return G * wgrad_splits(N, K, R, G) * (N * K + N);
}

RK_API int rk_gemm_wgrad_grouped(int32_t G, int64_t N, int64_t K, int64_t R, const float* const* A, int64_t lda,
                                 const float* const* B, int64_t ldb, float* const* C, int64_t ldc,
                                 float* const* row_sums, int32_t accumulate, float* workspace,
                                 int64_t workspace_floats, void* stream) {
  if (G <= 0 || N <= 0 || K <= 0 || R < 0 || !A || !B || !C || ldc < K || lda < N || ldb < K)
    return fail(RK_ERR_INVALID, "rk_gemm_wgrad_grouped: bad shape / operand");
  if (G > kWgMaxGroups) return fail(RK_ERR_UNSUPPORTED, "rk_gemm_wgrad_grouped: %d groups (<= %d)", G, kWgMaxGroups);
  WgradGroups gp = {};
  uintptr_t align = reinterpret_cast<uintptr_t>(workspace);
  for (int g = 0; g < G; ++g) {
    if (!C[g] || (R > 0 && (!A[g] || !B[g])) || (row_sums && !row_sums[g]))
      return fail(RK_ERR_INVALID, "rk_gemm_wgrad_grouped: group %d: null operand", g);
    gp.A[g] = A[g];
    gp.B[g] = B[g];
    gp.C[g] = C[g];
    gp.row_sums[g] = row_sums ? row_sums[g] : nullptr;
    align |= reinterpret_cast<uintptr_t>(A[g]) | reinterpret_cast<uintptr_t>(B[g]) | reinterpret_cast<uintptr_t>(C[g]) |
             reinterpret_cast<uintptr_t>(gp.row_sums[g]);
  }
  if ((N | K | lda | ldb | ldc) % 4 || (align & 15))
    return fail(RK_ERR_UNSUPPORTED, "rk_gemm_wgrad_grouped: needs N, K, lda, ldb, ldc multiples of 4 and 16-B "
                                    "aligned pointers");
  const int64_t need = rk_gemm_wgrad_grouped_workspace_floats(G, N, K, R);
  if (!workspace || workspace_floats < need)
    return fail(RK_ERR_INVALID, "rk_gemm_wgrad_grouped: workspace of %lld floats, needs %lld",
                (long long)workspace_floats, (long long)need);
  hipStream_t st = (hipStream_t)stream;
  const int64_t S = wgrad_splits(N, K, R, G);
  int64_t rps = (R + S - 1) / S;
  rps = std::max<int64_t>(kWgR, (rps + kWgR - 1) / kWgR * kWgR);
  const int64_t splits = std::max<int64_t>(1, (R + rps - 1) / rps);
  const int64_t ws_group = S * (N * K + N);  // splits <= S
  const int64_t tiles = ((N + kWgT - 1) / kWgT) * ((K + kWgT - 1) / kWgT);
  if (tiles > 65535) return fail(RK_ERR_UNSUPPORTED, "rk_gemm_wgrad_grouped: output too large");
  if (R > 0) {
    const dim3 grid((unsigned)splits, (unsigned)tiles, (unsigned)G);
    wgrad_grouped_kernel<<<grid, kWgThreads, 0, st>>>(gp, N, K, R, rps, lda, ldb, workspace, ws_group, splits,
                                                      row_sums != nullptr);
  } else {
    (void)hipMemsetAsync(workspace, 0, sizeof(float) * (size_t)(G * ws_group), st);
  }
  const int64_t c_blocks = (N * K / 4 + 63) / 64;
  const int64_t b_blocks = row_sums ? (N / 4 + 63) / 64 : 0;
  const dim3 rgrid((unsigned)(c_blocks + b_blocks), (unsigned)G);
  wgrad_reduce_grouped_kernel<<<rgrid, 1024, 0, st>>>(gp, workspace, ws_group, R > 0 ? splits : 1, N, K, ldc, accumulate,
                                                      c_blocks);
  return check_launch("rk_gemm_wgrad_grouped");
}
