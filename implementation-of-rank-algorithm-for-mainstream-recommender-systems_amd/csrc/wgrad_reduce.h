// The body of wgrad.hip's fixed-order slab reduction, included by wgrad_reduce_kernel and by
// wgrad_reduce_grouped_kernel (see wgrad_tile.h for why it is an inclusion).  The including kernel provides
// ws, wsb, S, N, K, C, ldc, row_sums, accumulate, c_blocks; blockIdx.x is the float4 block.
  __shared__ f32x4 red[16][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const bool bias = blockIdx.x >= c_blocks;
  const int64_t count4 = bias ? N / 4 : N * K / 4;
  const int64_t e = (bias ? blockIdx.x - c_blocks : blockIdx.x) * 64 + lane;  // float4 index
  const float* src = bias ? wsb : ws;
  const int64_t stride = bias ? N : N * K;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (e < count4) {
#pragma unroll 4
    for (int64_t sp = w; sp < S; sp += 16) s += *reinterpret_cast<const f32x4*>(src + sp * stride + 4 * e);
  }
  red[w][lane] = s;
  __syncthreads();
  if (w == 0 && e < count4) {
    f32x4 t = red[0][lane];
#pragma unroll
    for (int i = 1; i < 16; ++i) t += red[i][lane];
    if (bias) {
      float* d = row_sums + 4 * e;
#pragma unroll
      for (int c = 0; c < 4; ++c) d[c] = accumulate ? d[c] + t[c] : t[c];
    } else {
      const int64_t n = (4 * e) / K, k = (4 * e) % K;  // K % 4 == 0: the 4 values share a row
      float* d = C + n * ldc + k;
#pragma unroll
      for (int c = 0; c < 4; ++c) d[c] = accumulate ? d[c] + t[c] : t[c];
    }
  }
