// What the kernels that gather their own input row share on top of mlp_core.h.  All three
// (rk_mlp_forward_gather in mlp.hip, mmoe.hip, ple.hip): the row's column map and the host check that
// fills it.  The two multi-task forwards (mmoe.hip, ple.hip): the per-layer dispatch of a 16-row
// workgroup of 16 waves, the register sink of an expert's last layer, and the mix into / walk over the
// per-task mixtures in LDS.
#pragma once
#include "mlp_core.h"

namespace rk {

// A gathered row of up to kRowCols columns from up to kRowSegs segments (rk_concat_gather's column
// map): column c comes from segment col_seg[c] (255: no segment, a zero) at its column col_off[c].
constexpr int kRowSegs = 16;
constexpr int kRowCols = 256;
struct RowMap {
  rk_segment segs[kRowSegs];
  uint8_t col_seg[kRowCols], col_off[kRowCols];
};

// Checks the segments of a row `width` columns wide and fills its map; `name` is the entry point in
// the error message.  The caller has checked nseg <= kRowSegs and width <= kRowCols.
inline int row_map_fill(RowMap& map, const rk_segment* segs, int nseg, int width, const char* name) {
  for (int c = 0; c < kRowCols; ++c) {
    map.col_seg[c] = 255;
    map.col_off[c] = 0;
  }
  for (int i = 0; i < nseg; ++i) {
    const rk_segment& sg = segs[i];
    if (!sg.src || sg.dim <= 0 || sg.out_col < 0 || sg.out_col + sg.dim > width || (sg.idx && sg.rows <= 0) ||
        sg.dim > 255)
      return fail(RK_ERR_INVALID, "%s: segment %d invalid", name, i);
    map.segs[i] = sg;
    for (int c = sg.out_col; c < sg.out_col + sg.dim; ++c) {  // the last covering segment wins
      map.col_seg[c] = (uint8_t)i;
      map.col_off[c] = (uint8_t)(c - sg.out_col);
    }
  }
  return RK_OK;
}

// mlp_layer's sink of an expert's last layer: the wave's finished tiles stay in registers.
// (One type per tile count: with one object for both, the compiler merged the two layer variants'
// epilogue stores behind a runtime index and kept the tiles in scratch.)
template <int TPW>
struct TileSink {
  f32x4_t z[TPW];
  __device__ __forceinline__ void take(int j, int r, int row, float v) { z[j][r] = v; }
};

// mlp_rows' per-layer dispatch: wave w owns column tiles w and w + 16; a wave without a tile takes
// part in the active waves' lockstep barriers.
__device__ __forceinline__ void mtl_prepare(LayerPipe& pipe, const rk_mlp_layer& L, int K, int wave, int lane) {
  const int nt = pad64(L.n) / 16, kch = pad64(K) / 16;
  if (wave + kMlpWaves < nt)
    pipe.prepare<2, 4>(L, kch, wave, lane);
  else if (wave < nt)
    pipe.prepare<1, 8>(L, kch, wave, lane);
}

__device__ __forceinline__ void mtl_layer(LayerPipe& pipe, const rk_mlp_layer& L, const float* in, int ldin, float* out,
                                          int ldout, int Kp, int wave, int lane) {
  const int ntiles = pad64(L.n) / 16;
  if (wave + kMlpWaves < ntiles) {
    mlp_layer<2, 1, 4, false>(pipe, L, in, ldin, out, ldout, Kp, wave, lane, 0, kMlpRows);
  } else if (wave < ntiles) {
    mlp_layer<1, 1, 8, false>(pipe, L, in, ldin, out, ldout, Kp, wave, lane, 0, kMlpRows);
  } else {
    for (int i = 0; i < (Kp / 16 - 1) / kMlpSyncChunks; ++i) mlp_sync_barrier();
  }
}

// The same with the output tiles left in z (zero for a tile the wave does not own), nothing in LDS.
__device__ __forceinline__ void mtl_layer_tiles(LayerPipe& pipe, const rk_mlp_layer& L, const float* in, int ldin,
                                                int Kp, int wave, int lane, f32x4_t (&z)[2]) {
  const int ntiles = pad64(L.n) / 16;
  z[0] = z[1] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  if (wave + kMlpWaves < ntiles) {
    TileSink<2> f;
    mlp_layer<2, 1, 4, false>(pipe, L, in, ldin, nullptr, 0, Kp, wave, lane, 0, kMlpRows, 0, 0, &f);
    z[0] = f.z[0];
    z[1] = f.z[1];
  } else if (wave < ntiles) {
    TileSink<1> f;
    mlp_layer<1, 1, 8, false>(pipe, L, in, ldin, nullptr, 0, Kp, wave, lane, 0, kMlpRows, 0, 0, &f);
    z[0] = f.z[0];
  } else {
    for (int i = 0; i < (Kp / 16 - 1) / kMlpSyncChunks; ++i) mlp_sync_barrier();
  }
}

// The lane index behind an empty asm, taken once per layer: what a layer derives from it (LDS and
// weight addresses, output offsets) is then computed where it is used.  Derived from `lane` itself
// the compiler hoists all of it out of the expert / task loops and spills it around every layer.
__device__ __forceinline__ int lane_now(int lane) {
  asm volatile("" : "+v"(lane));
  return lane;
}

// The barrier that ends a layer (the next layer's weight ring was issued before it).
__device__ __forceinline__ void close_layer() {
  mlp_lds_barrier();
  __builtin_amdgcn_s_setprio(0);
}

// The mixtures mt [slots][Hp][16] (mt[(slot Hp + n) 16 + row]) hold every element in the MFMA
// accumulator layout, the 4 rows of a register quadruple contiguous, so each belongs to one lane: a
// conflict-free 16-byte read and write per tile, and no barrier guards them.
//
// The mix behind an expert's last layer: the lane adds g[row] * z, z the wave's finished tiles, into
// its own elements of mixture `slot`; the gate weights are column gcol of gt [columns][16].  `first`:
// the mixture's first expert, nothing is read.
__device__ __forceinline__ void mtl_mix(float* mt, const float* gt, int slot, int gcol, bool first,
                                        const f32x4_t (&z)[2], int Hp, int wave, int lane) {
  const int q4 = (lane >> 4) * 4;  // the lane's first row
  const f32x4_t gv = *reinterpret_cast<const f32x4_t*>(gt + gcol * kMlpRows + q4);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int t = wave + kMlpWaves * j;
    if (t < Hp / 16) {
      f32x4_t* const mp = reinterpret_cast<f32x4_t*>(mt + (slot * Hp + 16 * t + (lane & 15)) * kMlpRows + q4);
      f32x4_t m = {0.f, 0.f, 0.f, 0.f};
      if (!first) m = *mp;
#pragma unroll
      for (int q = 0; q < 4; ++q) m[q] = __builtin_fmaf(gv[q], z[j][q], m[q]);
      *mp = m;
    }
  }
}

// The walk back: f(row, n, value) for each of the lane's own elements of mixture `slot` (columns up
// to Hp: the pad columns hold zeros).
template <class F>
__device__ __forceinline__ void mtl_unmix(const float* mt, int slot, int Hp, int wave, int lane, F&& f) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int t = wave + kMlpWaves * j;
    if (t < Hp / 16) {
      const int n = 16 * t + (lane & 15);
      const f32x4_t mv = *reinterpret_cast<const f32x4_t*>(mt + (slot * Hp + n) * kMlpRows + (lane >> 4) * 4);
#pragma unroll
      for (int q = 0; q < 4; ++q) f((lane >> 4) * 4 + q, n, mv[q]);
    }
  }
}

}  // namespace rk
