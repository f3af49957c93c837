// cell_grid.hip -- the marked cells of a boundary-cell grid (cell_grid.h) on gfx950, built in one place for T3 (geometry
// smoothing, post_reconstruct.hip) and T6 (colour smoothing, color_smoothing.hip): addGridCentroid / addGridColorCentroid
// (PCCCodec.cpp:982-1000, :1170-1191) name a cell on first touch; here a cell's name is its rank in raster order.
#include "cell_grid.h"
#include "internal.h"

namespace tmc2 {
namespace {
__global__ __launch_bounds__( 256 ) void markCellsKernel( const Pt* __restrict__ pts, const uint8_t* __restrict__ btype, uint32_t M, CellGrid g,
                                                           uint32_t* __restrict__ bits ) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if ( i >= M || btype[i] != 1 ) return;
  const Pt p = pts[i];
  if ( g.outside( p.x, p.y, p.z ) ) return;  // (inside the faces and gridSize even: the eight cells lie in the grid)
  const int qx = g.lowerCell( p.x ), qy = g.lowerCell( p.y ), qz = g.lowerCell( p.z );
  for ( int k = 0; k < 8; ++k ) {
    const uint32_t key = g.key( qx + ( k & 1 ), qy + ( ( k >> 1 ) & 1 ), qz + ( k >> 2 ) );
    const uint32_t bit = 1u << ( key & 31u );
    if ( !( loadStaleOk( &bits[key >> 5] ) & bit ) ) atomicOr( &bits[key >> 5], bit );  // bits only ever get set
  }
}

__global__ __launch_bounds__( 256 ) void popcountWordsKernel( const uint32_t* __restrict__ bits, uint32_t* __restrict__ rank, uint32_t words ) {
  for ( uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < words; i += gridDim.x * blockDim.x ) rank[i] = __popc( bits[i] );
}
}  // namespace

int markedCells( tmc2_ctx* ctx, const Pt* d_pts, const uint8_t* d_btype, uint32_t M, const CellGrid& g, uint32_t* d_total, MarkedCells& out ) {
  hipStream_t s = ctx->stream;
  out.words     = uint32_t( ( g.cells() + 31 ) / 32 );
  TMC2_TRY( out.bits.alloc( out.words ) );
  TMC2_TRY( out.rank.alloc( out.words ) );
  TMC2_HIP( hipMemsetAsync( out.bits.p, 0, size_t( out.words ) * 4, s ) );
  if ( M ) hipLaunchKernelGGL( markCellsKernel, dim3( ( M + 255 ) / 256 ), dim3( 256 ), 0, s, d_pts, d_btype, M, g, out.bits.p );
  hipLaunchKernelGGL( popcountWordsKernel, dim3( cappedBlocks( ctx, ( out.words + 255 ) / 256 ) ), dim3( 256 ), 0, s, out.bits.p, out.rank.p,
                      out.words );
  TMC2_TRY( exclusiveScanU32( ctx, out.rank.p, out.rank.p, out.words, d_total ) );
  TMC2_HIP( hipMemcpyAsync( &out.count, d_total, 4, hipMemcpyDeviceToHost, s ) );
  TMC2_HIP( hipStreamSynchronize( s ) );
  return TMC2_OK;
}

}  // namespace tmc2
