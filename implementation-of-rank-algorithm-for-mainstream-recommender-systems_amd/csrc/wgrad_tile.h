// The body of the weight-gradient kernels of wgrad.hip, included once per kernel: wgrad_kernel (one
// problem) and wgrad_grouped_kernel (G problems) are the same code over different ways of finding the
// operands.  Textual inclusion, not a shared __device__ function: with the body inlined from a function
// the compiler scheduled rk_gemm_wgrad's kernels differently (127 / 142 VGPRs against 128 / 144, other
// instruction order), and that kernel's device code is meant to stay what was measured.
// The including kernel provides: N, K, R, rps, A, lda, A_mask, B, ldb, ws, wsb (the names of
// wgrad_kernel's parameters), the template flag MASK, and the macros RK_WG_TILE_N / RK_WG_TILE_K (its n and
// k tile index); blockIdx.x is the row slab.
  __shared__ float As2[2][kWgT * kWgP];  // double-buffered k-major images (139 KB, one workgroup per CU)
  __shared__ float Bs2[2][kWgT * kWgP];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wm = w & 3, wk = w >> 2;
#ifdef RK_WGRAD_STAMP  // diagnostic build only (tools/wgrad_clock.cpp): per-workgroup clock stamps
  uint64_t t0 = 0, r0s = 0;
  if (tid == 0) {
    t0 = __builtin_amdgcn_s_memtime();
    r0s = __builtin_amdgcn_s_memrealtime();
  }
  __builtin_amdgcn_s_waitcnt(0xC07F);
#endif
  const int n0 = RK_WG_TILE_N * kWgT, k0 = RK_WG_TILE_K * kWgT;
  const int64_t rb = (int64_t)blockIdx.x * rps;
  const int64_t re = min<int64_t>(R, rb + rps);
  f32x16 acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
  f32x4 bsum = {0.f, 0.f, 0.f, 0.f};
  const bool sums = wsb && RK_WG_TILE_K == 0;
  f32x4 va[4], vb[4], ma[4], mb[4];
  // lane half h = lane >> 5 takes reduction rows 8g + 4h + e at MFMA e of row group g (the same rows
  // for the A and B operands, so the k-permutation cancels in the sum)
  const int a_off = (32 * wm + (lane & 31)) * kWgP + 4 * (lane >> 5);
  const int b_off = (64 * wk + (lane & 31)) * kWgP + 4 * (lane >> 5);
  // prologue: step 0 into buffer 0, step 1's loads in flight
  wg_load<MASK>(A, lda, A_mask, rb, re, n0, (int)N, tid, va, ma);
  wg_load<false>(B, ldb, nullptr, rb, re, k0, (int)K, tid, vb, mb);
  if (sums)
    wg_store<MASK, true>(As2[0], tid, va, ma, rb, re, n0, (int)N, bsum);
  else
    wg_store<MASK, false>(As2[0], tid, va, ma, rb, re, n0, (int)N, bsum);
  wg_store<false, false>(Bs2[0], tid, vb, mb, rb, re, k0, (int)K, bsum);
  if (rb + kWgR < re) {
    wg_load<MASK>(A, lda, A_mask, rb + kWgR, re, n0, (int)N, tid, va, ma);
    wg_load<false>(B, ldb, nullptr, rb + kWgR, re, k0, (int)K, tid, vb, mb);
  }
  __syncthreads();
  int cb = 0;
  // one barrier per step: step s computes from buffer s & 1 while step s + 1's rows (loaded during
  // step s - 1) are written into the other buffer between the MFMA groups
  for (int64_t r0 = rb; r0 < re; r0 += kWgR, cb ^= 1) {
    const float* a_col = As2[cb] + a_off;
    const float* b_col = Bs2[cb] + b_off;
    const bool more = r0 + kWgR < re;
    f32x4 a[2], b0[2], b1[2];
    a[0] = *reinterpret_cast<const f32x4*>(a_col);
    b0[0] = *reinterpret_cast<const f32x4*>(b_col);
    b1[0] = *reinterpret_cast<const f32x4*>(b_col + 32 * kWgP);
#pragma unroll
    for (int g = 0; g < kWgR / 8; ++g) {
      const int cur = g & 1, nxt = cur ^ 1;
      if (g + 1 < kWgR / 8) {
        a[nxt] = *reinterpret_cast<const f32x4*>(a_col + 8 * (g + 1));
        b0[nxt] = *reinterpret_cast<const f32x4*>(b_col + 8 * (g + 1));
        b1[nxt] = *reinterpret_cast<const f32x4*>(b_col + 32 * kWgP + 8 * (g + 1));
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc0 = mfma32(a[cur][e], b0[cur][e], acc0);
        acc1 = mfma32(a[cur][e], b1[cur][e], acc1);
      }
      if (g == 1 && more) {  // the next step's rows have had a whole step to arrive
        if (sums)
          wg_store<MASK, true>(As2[cb ^ 1], tid, va, ma, r0 + kWgR, re, n0, (int)N, bsum);
        else
          wg_store<MASK, false>(As2[cb ^ 1], tid, va, ma, r0 + kWgR, re, n0, (int)N, bsum);
        wg_store<false, false>(Bs2[cb ^ 1], tid, vb, mb, r0 + kWgR, re, k0, (int)K, bsum);
        if (r0 + 2 * kWgR < re) {
          wg_load<MASK>(A, lda, A_mask, r0 + 2 * kWgR, re, n0, (int)N, tid, va, ma);
          wg_load<false>(B, ldb, nullptr, r0 + 2 * kWgR, re, k0, (int)K, tid, vb, mb);
        }
      }
    }
    __syncthreads();
  }
  // partial tile: lane holds C[n0 + 32 wm + acc_row(r)][k0 + 64 wk + (lane & 31) (+32)]
  float* out = ws + (int64_t)blockIdx.x * N * K;
  const int64_t k = k0 + 64 * wk + (lane & 31);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t n = n0 + 32 * wm + acc_row(r, lane);
    if (n < N) {
      if (k < K) out[n * K + k] = acc0[r];
      if (k + 32 < K) out[n * K + k + 32] = acc1[r];
    }
  }
#ifdef RK_WGRAD_STAMP
  if (tid == 0) {
    const uint64_t t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    extern __device__ uint64_t g_wgrad_stamp[];
    uint64_t* st = g_wgrad_stamp + 4 * (blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z));
    st[0] = t0; st[1] = t1; st[2] = r0s; st[3] = r1;
  }
#endif
  if (sums) {  // fold the 16 row groups holding the same four columns (threads t, t + 32, ...)
    __syncthreads();
    float* red = As2[0];  // [16][128]
    *reinterpret_cast<f32x4*>(red + (tid >> 5) * kWgT + 4 * (tid & 31)) = bsum;
    __syncthreads();
    if (tid < kWgT && n0 + tid < N) {
      float s = 0.f;
#pragma unroll
      for (int g = 0; g < 16; ++g) s += red[g * kWgT + tid];
      wsb[(int64_t)blockIdx.x * N + n0 + tid] = s;
    }
  }
