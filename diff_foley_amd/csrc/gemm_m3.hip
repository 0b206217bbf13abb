// Instantiations of the implicit-GEMM kernel (gemm_impl.h), MODE 3 (the GEN rows of gemm_tiles.def that have M3): nearest-x2
// upsample + conv3x3 evaluated as four 2x2-tap convolutions on the INPUT-resolution map, one per output phase (Y & 1, X & 1), with
// per-phase weights that are the sums of the 3x3 taps falling on the same input pixel (openai_unetmodel.py:100-119 Upsample; 16
// instead of 36 multiply-adds per input pixel).
#include "gemm_impl.h"

hipError_t launch_gemm_m3(int tile_cfg, int epi, const GemmParams& p, int zdim, hipStream_t stream) {
#define DF_T(T, BM, BN, WGM, WGN, NST)                                     \
  case T:                                                                \
    switch (epi) {                                                       \
      case EPI_LEAN: return launch_cfg<BM, BN, WGM, WGN, NST, 3, EPI_LEAN>(p, zdim, stream); \
      case EPI_SPLITK: return launch_cfg<BM, BN, WGM, WGN, NST, 3, EPI_SPLITK>(p, zdim, stream); \
      case EPI_ANY: return launch_cfg<BM, BN, WGM, WGN, NST, 3, EPI_ANY>(p, zdim, stream); \
      default: return hipErrorInvalidValue;                              \
    }
#define DF_TILE_GEN0(T, M0, M1, M2, M3, BM, BN, WGM, WGN, NST, PS, LNS) DF_TILE_IF_##M3(DF_T(T, BM, BN, WGM, WGN, NST))
#define DF_TILE_GEN1(T, M0, M1, M2, M3, BM, BN, WGM, WGN, NST, PS, LNS) DF_TILE_IF_##M3(DF_T(T, BM, BN, WGM, WGN, NST))
  switch (tile_cfg) {
#include "gemm_tiles.def"
    default: return hipErrorInvalidValue;
  }
#undef DF_T
}
