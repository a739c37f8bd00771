// The 128x128 MFMA tile loop shared by the ViT GEMM (gemm.hip) and the all-rows lm_head of the
// teacher-forced scoring call (score.hip):  acc[128,128] += A[m0.., K-tiles] . W[n0.., K-tiles]^T.
//
// 256 threads = 4 waves in 2x2, each wave 64x64 = 4x4 MFMA 16x16 tiles.  K step = 128 bytes per row
// (64 bf16 / f16 or 32 f32).  Operands stream global->LDS with global_load_lds_dwordx4 (1 KiB per
// wave instruction, lane-linear LDS image); the st_8x16B XOR swizzle (chunk ^ (row & 7)) is applied on
// the global SOURCE address and on the ds_read address, making the ds_read_b128 fragment reads
// conflict-free.  Both operands are K-contiguous ([rows, K] row-major).
#pragma once
#include "vcap_common.h"

namespace gemm_tile {

constexpr int BM = 128, BN = 128, ROWB = 128;  // ROWB: bytes of K per tile row
constexpr int TILE_BYTES = BM * ROWB;          // 16 KiB per operand per stage
constexpr int STAGE_BYTES = 2 * TILE_BYTES;

VCAP_DEV void glds16(const void* g, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// rows past `rows` re-read row rows - 1 (their results are the caller's to discard)
template <typename T>
VCAP_DEV void stage_tile(const T* __restrict__ P, long ld, int row0, int rows, int k0, char* lds_tile,
                         int wave, int lane) {
  constexpr int E = Frag<T>::kElems;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int rb = wave * 4 + i;              // 8-row block written by this wave instruction
    const int r = rb * 8 + (lane >> 3);
    const int s = lane & 7;                   // LDS slot within the 128-byte row
    const int c = s ^ (r & 7);                // global chunk stored in that slot
    int gr = row0 + r;
    gr = gr < rows ? gr : rows - 1;
    const T* src = P + (long)gr * ld + k0 + c * E;
    glds16(src, lds_tile + rb * 1024);
  }
}

VCAP_DEV u32x4 lds_frag(const char* tile, int row, int chunk) {
  return *reinterpret_cast<const u32x4*>(tile + row * ROWB + ((chunk ^ (row & 7)) << 4));
}

// K-tiles [kt0, kt0 + nk) of the tile at (m0, n0), double-buffered through smem (2 * STAGE_BYTES).
// The weight fragment is the MFMA A operand, so lane (fr = lane & 15, fg = lane >> 4) of wave
// (wm = wave >> 1, wn = wave & 1) ends up with acc[i][j][e] = C[m0 + wm*64 + i*16 + fr][n0 + wn*64 +
// j*16 + 4*fg + e]: 4 consecutive COLUMNS of one row (vector stores in the epilogue).  Returns after
// a workgroup barrier: smem is free again.
template <typename TIn>
VCAP_DEV void tile_loop(const TIn* __restrict__ A, long lda, const TIn* __restrict__ W, long ldw, int m0, int M,
                        int n0, int N, int kt0, int nk, char* smem, f32x4 (&acc)[4][4]) {
  constexpr int BK = ROWB / sizeof(TIn);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  stage_tile(A, lda, m0, M, kt0 * BK, smem, wave, lane);
  stage_tile(W, ldw, n0, N, kt0 * BK, smem + TILE_BYTES, wave, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const int fr = lane & 15, fg = lane >> 4;
  for (int kt = 0; kt < nk; ++kt) {
    char* cur = smem + (kt & 1) * STAGE_BYTES;
    if (kt + 1 < nk) {
      char* nxt = smem + ((kt + 1) & 1) * STAGE_BYTES;
      stage_tile(A, lda, m0, M, (kt0 + kt + 1) * BK, nxt, wave, lane);
      stage_tile(W, ldw, n0, N, (kt0 + kt + 1) * BK, nxt + TILE_BYTES, wave, lane);
    }
    const char* ta = cur;
    const char* tb = cur + TILE_BYTES;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      u32x4 af[4], bfr[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = lds_frag(ta, wm * 64 + i * 16 + fr, s * 4 + fg);
#pragma unroll
      for (int j = 0; j < 4; ++j) bfr[j] = lds_frag(tb, wn * 64 + j * 16 + fr, s * 4 + fg);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = mfma_frag(bfr[j], af[i], acc[i][j], (TIn*)nullptr);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
}

}  // namespace gemm_tile
