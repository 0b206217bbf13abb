// Instantiations of the implicit-GEMM kernel (gemm_impl.h), MODE 0: the GEN rows of gemm_tiles.def, part 1.  One translation unit per
// mode (MODE 0: two) so they build in parallel.
#include "gemm_impl.h"

hipError_t launch_gemm_m0b(int tile_cfg, int epi, const GemmParams& p, int zdim, hipStream_t stream) {
#define DF_T(T, BM, BN, WGM, WGN, NST)                                     \
  case T:                                                                \
    switch (epi) {                                                       \
      case EPI_LEAN: return launch_cfg<BM, BN, WGM, WGN, NST, 0, EPI_LEAN>(p, zdim, stream); \
      case EPI_SPLITK: return launch_cfg<BM, BN, WGM, WGN, NST, 0, EPI_SPLITK>(p, zdim, stream); \
      case EPI_GEGLU: return launch_cfg<BM, BN, WGM, WGN, NST, 0, EPI_GEGLU>(p, zdim, stream); \
      case EPI_PROD: return launch_cfg<BM, BN, WGM, WGN, NST, 0, EPI_PROD>(p, zdim, stream); \
      case EPI_LNC: return launch_cfg<BM, BN, WGM, WGN, NST, 0, EPI_LNC>(p, zdim, stream); \
      case EPI_ANY: return launch_cfg<BM, BN, WGM, WGN, NST, 0, EPI_ANY>(p, zdim, stream); \
      case EPI_XS: return launch_cfg<BM, BN, WGM, WGN, NST, 0, EPI_XS>(p, zdim, stream); \
      default: return hipErrorInvalidValue;                              \
    }
#define DF_TILE_GEN1(T, M0, M1, M2, M3, BM, BN, WGM, WGN, NST, PS, LNS) DF_TILE_IF_##M0(DF_T(T, BM, BN, WGM, WGN, NST))
  switch (tile_cfg) {
#include "gemm_tiles.def"
    default: return hipErrorInvalidValue;
  }
#undef DF_T
}
