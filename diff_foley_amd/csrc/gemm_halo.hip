// Instantiations of the halo conv3x3 kernel (gemm_impl.h): the HALO rows of gemm_tiles.def.
#include "gemm_impl.h"

hipError_t launch_gemm_halo(int tile_cfg, int epi, const GemmParams& p, int zdim, size_t lds, hipStream_t stream) {
#define DF_TILE_HALO0(T, M0, M1, M2, M3, BM, BN, WGM, WGN, NSTW, PS, LNS)                             \
  static_assert(!(M0) && (M1) && !(M2) && !(M3), "a halo tile is a stride-1 conv3x3 kernel: MODE 1"); \
  case T: \
    switch (epi) {                                                                                    \
      case EPI_LEAN: return launch_halo<BM, BN, WGM, WGN, NSTW, EPI_LEAN, PS>(p, zdim, lds, stream);  \
      case EPI_SPLITK: return launch_halo<BM, BN, WGM, WGN, NSTW, EPI_SPLITK, PS>(p, zdim, lds, stream); \
      case EPI_ANY: return launch_halo<BM, BN, WGM, WGN, NSTW, EPI_ANY, PS>(p, zdim, lds, stream);    \
      default: return hipErrorInvalidValue;                                                           \
    }
  switch (tile_cfg) {
#include "gemm_tiles.def"
    default: return hipErrorInvalidValue;
  }
}
