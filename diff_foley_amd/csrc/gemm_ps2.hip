// Instantiations of the implicit-GEMM kernel (gemm_impl.h) with PRODUCER-SPECIALISED blocks, MODE 0 and 1: the PS rows of
// gemm_tiles.def, part 1 (the small tiles).
#include "gemm_impl.h"

hipError_t launch_gemm_ps_small(int mode, int tile_cfg, int epi, const GemmParams& p, int zdim, hipStream_t stream) {
#define DF_TILE_PS1(T, M0, M1, M2, M3, BM, BN, WGM, WGN, NST, PS, LNS)                                  \
  static_assert((M0) && (M1) && !(M2) && !(M3), "producer-specialised tiles are built for MODE 0 and 1"); \
  case T: \
    if (mode == 1) switch (epi) {                                                                      \
      case EPI_LEAN: return launch_cfg<BM, BN, WGM, WGN, NST, 1, EPI_LEAN, NST, PS>(p, zdim, stream);  \
      case EPI_SPLITK: return launch_cfg<BM, BN, WGM, WGN, NST, 1, EPI_SPLITK, NST, PS>(p, zdim, stream); \
      case EPI_ANY: return launch_cfg<BM, BN, WGM, WGN, NST, 1, EPI_ANY, NST, PS>(p, zdim, stream);    \
      default: return hipErrorInvalidValue;                                                            \
    }                                                                                                  \
    if (mode != 0) return hipErrorInvalidValue;                                                        \
    switch (epi) {                                                                                     \
      case EPI_LEAN: return launch_cfg<BM, BN, WGM, WGN, NST, 0, EPI_LEAN, NST, PS>(p, zdim, stream);  \
      case EPI_SPLITK: return launch_cfg<BM, BN, WGM, WGN, NST, 0, EPI_SPLITK, NST, PS>(p, zdim, stream); \
      case EPI_GEGLU: return launch_cfg<BM, BN, WGM, WGN, NST, 0, EPI_GEGLU, NST, PS>(p, zdim, stream); \
      case EPI_PROD: return launch_cfg<BM, BN, WGM, WGN, NST, 0, EPI_PROD, NST, PS>(p, zdim, stream);  \
      case EPI_LNC: return launch_cfg<BM, BN, WGM, WGN, NST, 0, EPI_LNC, NST, PS>(p, zdim, stream);    \
      case EPI_ANY: return launch_cfg<BM, BN, WGM, WGN, NST, 0, EPI_ANY, NST, PS>(p, zdim, stream);    \
      case EPI_XS: return launch_cfg<BM, BN, WGM, WGN, NST, 0, EPI_XS, NST, PS>(p, zdim, stream);      \
      default: return hipErrorInvalidValue;                                                            \
    }
  switch (tile_cfg) {
#include "gemm_tiles.def"
    default: return hipErrorInvalidValue;
  }
}
