// Instantiations of the implicit-GEMM kernel (gemm_impl.h), MODE 2: the GEN rows of gemm_tiles.def that have M2.  One translation
// unit per mode (MODE 0: two) so they build in parallel.
#include "gemm_impl.h"

hipError_t launch_gemm_m2(int tile_cfg, int epi, const GemmParams& p, int zdim, hipStream_t stream) {
#define DF_T(T, BM, BN, WGM, WGN, NST)                                     \
  case T:                                                                \
    switch (epi) {                                                       \
      case EPI_LEAN: return launch_cfg<BM, BN, WGM, WGN, NST, 2, EPI_LEAN>(p, zdim, stream); \
      case EPI_SPLITK: return launch_cfg<BM, BN, WGM, WGN, NST, 2, EPI_SPLITK>(p, zdim, stream); \
      case EPI_ANY: return launch_cfg<BM, BN, WGM, WGN, NST, 2, EPI_ANY>(p, zdim, stream); \
      default: return hipErrorInvalidValue;                              \
    }
#define DF_TILE_GEN0(T, M0, M1, M2, M3, BM, BN, WGM, WGN, NST, PS, LNS) DF_TILE_IF_##M2(DF_T(T, BM, BN, WGM, WGN, NST))
#define DF_TILE_GEN1(T, M0, M1, M2, M3, BM, BN, WGM, WGN, NST, PS, LNS) DF_TILE_IF_##M2(DF_T(T, BM, BN, WGM, WGN, NST))
  switch (tile_cfg) {
#include "gemm_tiles.def"
    default: return hipErrorInvalidValue;
  }
#undef DF_T
}
