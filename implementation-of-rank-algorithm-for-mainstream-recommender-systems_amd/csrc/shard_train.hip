// The local steps of ShardedDeepFM's training step around its all-to-alls (rankops/sharded.py,
// DESIGN.md §7; the reference trains DeepFM on one device, deepfm.py:153-201 — the hybrid-parallel
// step is this build's own).  The wire is the split format of rk_shard_gather_rows_split, forward
// and backward: per (source, owner) a block of [B][F_r][D] rows, then pad4(B) first-order floats.
// Fields are dealt round robin: field f lives on owner f % P at slot f / P, so owner r holds
// F_r = F / P + (r < F % P) fields and every block offset is a closed form of (r, B, F, P, D) —
// no descriptor tables, no limit on P.
//
//  rk_shard_fm_assemble       receiver, forward: the blocks of all owners -> the deep input
//                             [B, F * D] in field order, fm1 = the owners' partials summed in owner
//                             order, fm2 = 0.5 * sum_d ((sum_f e)^2 - sum_f e^2).
//  rk_shard_fm_backward_pack  receiver, backward: the FM backward (rk_fm_backward's arithmetic,
//                             train_common.h) written straight into the gradient send blocks, with
//                             scale * dfm1 in every owner's tail and zeros in the tail's pad lanes.
//  rk_shard_unpack_grads      owner, backward: the received gradient blocks [s][B][F_me][D] + tails
//                             and the kept int32 indices [s][B][F_me] -> per local table the COO
//                             pieces ids int64 [N], values2 [N, D] (N = P * B, entry s * B + b) and
//                             one shared first-order values vector [N].
//
// All three are byte movers bound by the request rate: D / 4 lanes per (sample,
// field) row with 16-B accesses (one 128-B request per row at D = 32), kShardTrainU rows in flight
// per lane group before the first use, 32-bit index arithmetic inside a sample and no 64-bit
// division anywhere (the source is grid.y where there is one), no float atomics.  Buffers the
// collective reads next are written with nontemporal stores.
#include "train_common.h"

namespace rk {

constexpr int kShardTrainU = 8;  // rows in flight per lane group

// The wire layout of one rank's send / receive buffer of P blocks.
struct ShardWire {
  int F, P, G;     // fields, owners, float4 quads per row (D / 4)
  int rem, Flo;    // F % P, F / P
  int owners;      // owners with at least one field: min(P, F)
  int64_t B, pad;  // samples per block, pad4(B)
  int64_t blk_hi, blk_lo;  // floats of a block with Flo + 1 / Flo fields (0 for an empty owner)

  __host__ __device__ int fields_of(int r) const { return Flo + (r < rem ? 1 : 0); }
  __host__ __device__ int64_t block_offset(int r) const {
    return r < rem ? r * blk_hi : rem * blk_hi + (int64_t)(r - rem) * blk_lo;
  }
};

static ShardWire make_wire(int F, int P, int dim, int64_t B) {
  ShardWire w;
  w.F = F;
  w.P = P;
  w.G = dim / 4;
  w.rem = F % P;
  w.Flo = F / P;
  w.owners = std::min(P, F);
  w.B = B;
  w.pad = (B + 3) & ~(int64_t)3;
  w.blk_hi = B * (w.Flo + 1) * dim + w.pad;
  w.blk_lo = w.Flo > 0 ? B * w.Flo * dim + w.pad : 0;
  return w;
}

struct ShardAssembleArgs {
  ShardWire w;
  const float* recv;
  float* deep_in;
  int64_t ld_deep;
  float* fm1;
  float* fm2;
};

// One lane group (G lanes) per sample: the F rows of the sample, kShardTrainU loads in flight,
// copied to the deep input and accumulated into sum and sum of squares per column; the groups'
// column partials of fm2 meet in LDS (G need not be a power of two) and the group's first lane
// adds them in lane order, then the owners' first-order partials in owner order.
__global__ __launch_bounds__(256) void shard_fm_assemble_kernel(ShardAssembleArgs a) {
  __shared__ float part[256];
  const ShardWire& w = a.w;
  const int G = w.G, D = 4 * G, S = 256 / G;
  const int tid = threadIdx.x, grp = tid / G, q = tid - grp * G;
  const int64_t b = (int64_t)blockIdx.x * S + grp;
  const bool live = grp < S && b < w.B;
  f32x4 s = {0.f, 0.f, 0.f, 0.f}, sq = {0.f, 0.f, 0.f, 0.f};
  if (live) {
    float* const dst = a.deep_in + b * a.ld_deep + 4 * q;
    int r = 0, j = 0;  // owner and slot of the next field
    for (int f0 = 0; f0 < w.F; f0 += kShardTrainU) {
      int64_t p[kShardTrainU];  // offsets into a.recv
#pragma unroll
      for (int u = 0; u < kShardTrainU; ++u) {
        p[u] = 0;
        if (f0 + u < w.F) {
          p[u] = w.block_offset(r) + (b * w.fields_of(r) + j) * D + 4 * q;
          if (++r == w.P) r = 0, ++j;
        }
      }
      f32x4 v[kShardTrainU];
#pragma unroll
      for (int u = 0; u < kShardTrainU; ++u)
        if (f0 + u < w.F) v[u] = *reinterpret_cast<const f32x4*>(a.recv + p[u]);
#pragma unroll
      for (int u = 0; u < kShardTrainU; ++u)
        if (f0 + u < w.F) {
          *reinterpret_cast<f32x4*>(dst + (f0 + u) * D) = v[u];
          s += v[u];
          sq += v[u] * v[u];
        }
    }
  }
  part[tid] = (s.x * s.x - sq.x) + (s.y * s.y - sq.y) + (s.z * s.z - sq.z) + (s.w * s.w - sq.w);
  __syncthreads();
  if (live && q == 0) {
    float t = 0.f;
    for (int i = 0; i < G; ++i) t += part[tid + i];
    a.fm2[b] = 0.5f * t;
    float fo = 0.f;
    for (int r = 0; r < w.owners; ++r) fo += a.recv[w.block_offset(r) + w.B * w.fields_of(r) * D + b];
    a.fm1[b] = fo;
  }
}

struct ShardGradPackArgs {
  ShardWire w;
  const float* deep_in;
  int64_t ld_in;
  const float* d_deep;
  int64_t ld_d;
  const float* dfm2;
  const float* dfm1;
  float scale;
  float* out;
};

// One lane group per sample: S over the sample's F rows (field order, fm_field_sum), then the
// rows again (on-die now) with d_deep's, kShardTrainU of each in flight, g = scale * fm_grad(...)
// stored past L2 into the owner's block.  The group's first lane writes the first-order tails;
// the last sample's also zeroes the pad lanes.
__global__ __launch_bounds__(256) void shard_fm_backward_pack_kernel(ShardGradPackArgs a) {
  const ShardWire& w = a.w;
  const int G = w.G, D = 4 * G, S = 256 / G;
  const int tid = threadIdx.x, grp = tid / G, q = tid - grp * G;
  const int64_t b = (int64_t)blockIdx.x * S + grp;
  if (grp >= S || b >= w.B) return;  // no barrier below
  const f32x4* const e = reinterpret_cast<const f32x4*>(a.deep_in + b * a.ld_in) + q;
  const f32x4* const dd = a.d_deep ? reinterpret_cast<const f32x4*>(a.d_deep + b * a.ld_d) + q : nullptr;
  const f32x4 Ssum = fm_field_sum(e, w.F, (int64_t)G);
  const float g2 = a.dfm2 ? a.dfm2[b] : 0.f;
  int r = 0, j = 0;
  for (int f0 = 0; f0 < w.F; f0 += kShardTrainU) {
    f32x4 ev[kShardTrainU], dv[kShardTrainU];
    int64_t o[kShardTrainU];  // offsets into a.out (a pointer per slot would lose the global address space)
#pragma unroll
    for (int u = 0; u < kShardTrainU; ++u) {
      o[u] = 0;
      dv[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (f0 + u < w.F) {
        ev[u] = e[(f0 + u) * G];
        if (dd) dv[u] = dd[(f0 + u) * G];
        o[u] = w.block_offset(r) + (b * w.fields_of(r) + j) * D + 4 * q;
        if (++r == w.P) r = 0, ++j;
      }
    }
#pragma unroll
    for (int u = 0; u < kShardTrainU; ++u)
      if (f0 + u < w.F)
        __builtin_nontemporal_store(a.scale * fm_grad(dv[u], g2, Ssum, ev[u]),
                                    reinterpret_cast<f32x4*>(a.out + o[u]));
  }
  if (q == 0) {
    const float t = a.dfm1[b] * a.scale;
    for (int rr = 0; rr < w.owners; ++rr) {
      float* const tail = a.out + w.block_offset(rr) + w.B * w.fields_of(rr) * D;
      tail[b] = t;
      if (b == w.B - 1)
        for (int64_t i = w.B; i < w.pad; ++i) tail[i] = 0.f;
    }
  }
}

struct ShardUnpackArgs {
  const float* recv;   // per source: [B][F][D] then pad4(B) first-order gradients
  const int32_t* idx;  // [P][B][F] as received in the forward
  int F, G;            // this owner's fields; quads per row
  int64_t B, N;        // samples per source; P * B
  int64_t* ids;        // [F][N]
  float* values2;      // [F][N][D]
  float* values1;      // [N]
};

// One lane group per (source, sample), the source in grid.y: the sample's F gradient rows,
// kShardTrainU loads in flight, to entry i = s * B + b of each table's value block; the ids widened
// by the group's lanes in turn (-1 stays -1), the shared first-order value by its first lane.
__global__ __launch_bounds__(256) void shard_unpack_grads_kernel(ShardUnpackArgs a) {
  const int G = a.G, D = 4 * G, S = 256 / G, F = a.F;
  const int tid = threadIdx.x, grp = tid / G, q = tid - grp * G;
  const int64_t b = (int64_t)blockIdx.x * S + grp;
  if (grp >= S || b >= a.B) return;  // no barrier below
  const int s = blockIdx.y;
  const int64_t blk = a.B * F * D + ((a.B + 3) & ~(int64_t)3);
  const float* const in = a.recv + s * blk;
  const int64_t i = s * a.B + b;
  const float* const rows = in + b * F * D + 4 * q;
  float* const out = a.values2 + i * D + 4 * q;
  for (int j0 = 0; j0 < F; j0 += kShardTrainU) {
    f32x4 v[kShardTrainU];
#pragma unroll
    for (int u = 0; u < kShardTrainU; ++u)
      if (j0 + u < F) v[u] = *reinterpret_cast<const f32x4*>(rows + (j0 + u) * D);
#pragma unroll
    for (int u = 0; u < kShardTrainU; ++u)
      if (j0 + u < F) *reinterpret_cast<f32x4*>(out + (j0 + u) * a.N * D) = v[u];
  }
  const int32_t* const ip = a.idx + i * F;
  for (int j = q; j < F; j += G) a.ids[j * a.N + i] = (int64_t)ip[j];
  if (q == 0) a.values1[i] = in[a.B * F * D + b];
}

static bool wire_ok(int F, int P, int dim, int64_t B) {
  return F > 0 && P > 0 && dim >= 4 && dim % 4 == 0 && dim <= 1024 && B >= 0 &&
         (F + P - 1) / P <= kShardMaxFields;
}

}  // namespace rk

using namespace rk;

RK_API int rk_shard_fm_assemble(const float* recv, int32_t num_fields, int32_t num_owners, int32_t dim,
                                int64_t batch, float* deep_in, int64_t ld_deep, float* fm1, float* fm2,
                                void* stream) {
  if (!wire_ok(num_fields, num_owners, dim, batch) || !recv || !deep_in || !fm1 || !fm2 ||
      ld_deep < (int64_t)num_fields * dim || ld_deep % 4 || !aligned16(recv) || !aligned16(deep_in))
    return fail(RK_ERR_INVALID, "rk_shard_fm_assemble: bad arguments (fields %d on %d owners, <= %d each; dim %d "
                                "%% 4 == 0; 16-B aligned buffers)", num_fields, num_owners, kShardMaxFields, dim);
  if (batch == 0) return RK_OK;
  ShardAssembleArgs a = {make_wire(num_fields, num_owners, dim, batch), recv, deep_in, ld_deep, fm1, fm2};
  const int S = 256 / a.w.G;
  shard_fm_assemble_kernel<<<(unsigned)((batch + S - 1) / S), 256, 0, (hipStream_t)stream>>>(a);
  return check_launch("rk_shard_fm_assemble");
}

RK_API int rk_shard_fm_backward_pack(const float* deep_in, int64_t ld_in, const float* d_deep, int64_t ld_d,
                                     const float* dfm2, const float* dfm1, float scale, int64_t batch,
                                     int32_t num_fields, int32_t num_owners, int32_t dim, float* out,
                                     void* stream) {
  if (!wire_ok(num_fields, num_owners, dim, batch) || !deep_in || !dfm1 || !out ||
      ld_in < (int64_t)num_fields * dim || ld_in % 4 || !aligned16(deep_in) ||
      (d_deep && (ld_d < (int64_t)num_fields * dim || ld_d % 4 || !aligned16(d_deep))) || !aligned16(out))
    return fail(RK_ERR_INVALID, "rk_shard_fm_backward_pack: bad arguments (fields %d on %d owners, <= %d each; dim "
                                "%d %% 4 == 0; 16-B aligned buffers)", num_fields, num_owners, kShardMaxFields,
                dim);
  if (batch == 0) return RK_OK;
  ShardGradPackArgs a = {make_wire(num_fields, num_owners, dim, batch), deep_in, ld_in, d_deep, ld_d, dfm2, dfm1, scale,
                      out};
  const int S = 256 / a.w.G;
  shard_fm_backward_pack_kernel<<<(unsigned)((batch + S - 1) / S), 256, 0, (hipStream_t)stream>>>(a);
  return check_launch("rk_shard_fm_backward_pack");
}

RK_API int rk_shard_unpack_grads(const float* recv, const int32_t* idx, int32_t num_fields, int32_t dim,
                                 int32_t num_sources, int64_t source_batch, int64_t* ids, float* values2,
                                 float* values1, void* stream) {
  if (num_fields < 0 || num_fields > kShardMaxFields || dim < 4 || dim % 4 || dim > 1024 || num_sources <= 0 ||
      num_sources > 65535 || source_batch < 0)
    return fail(RK_ERR_INVALID, "rk_shard_unpack_grads: bad arguments (fields %d <= %d, dim %d %% 4 == 0, %d sources)",
                num_fields, kShardMaxFields, dim, num_sources);
  if (num_fields == 0) return RK_OK;  // an owner without fields (world > fields) receives nothing
  if (!recv || !idx || !ids || !values2 || !values1 || !aligned16(recv) || !aligned16(values2) ||
      ((uintptr_t)ids & 7u))
    return fail(RK_ERR_INVALID, "rk_shard_unpack_grads: buffers must be non-null (rows 16-B, ids 8-B aligned)");
  if (source_batch == 0) return RK_OK;
  ShardUnpackArgs a = {recv, idx, num_fields, dim / 4, source_batch, (int64_t)num_sources * source_batch, ids,
                       values2, values1};
  const int S = 256 / a.G;
  const dim3 grid((unsigned)((source_batch + S - 1) / S), (unsigned)num_sources);
  shard_unpack_grads_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(a);
  return check_launch("rk_shard_unpack_grads");
}
