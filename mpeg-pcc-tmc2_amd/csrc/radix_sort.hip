// radix_sort.hip -- stable LSD radix sort of (64-bit key, 32-bit payload) pairs on gfx950.  Shared by the metric's lexicographic
// de-duplication (metrics.hip: removeDuplicatesDevice) and the voxelisation of the grid-based segmentation (voxelize.hip): in a
// STABLE sort of (key, input index) pairs the first element of a run of equal keys is the one with the smallest input index.
// Both mark those first elements next (markRunHeads).
#include "internal.h"
#include "wave.h"

namespace tmc2 {
namespace {
// Stable LSD radix sort, 8 bits per pass, tiles of kSortTile keys per workgroup: per-tile digit counts (radixCountKernel), one
// prefix sum over counts[digit][tile] (digit-major: the exclusive sum IS the digit's base plus the tiles before), then the
// scatter: a tile is ranked in sub-tiles of 256 keys -- within a wavefront the lanes holding the same digit find each other
// with eight ballots, the waves' counts are prefixed through LDS, running per-digit offsets carry over the sub-tiles.
constexpr int kSortTile = 2048;
__global__ __launch_bounds__( 256 ) void radixCountKernel( const uint64_t* __restrict__ key, uint32_t n, int shift, uint32_t tiles,
                                                            uint32_t* __restrict__ counts ) {
  __shared__ uint32_t bins[256];
  bins[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t base = blockIdx.x * kSortTile;
  for ( uint32_t i = base + threadIdx.x; i < min( n, base + uint32_t( kSortTile ) ); i += 256 ) atomicAdd( &bins[( key[i] >> shift ) & 0xFF], 1u );
  __syncthreads();
  counts[size_t( threadIdx.x ) * tiles + blockIdx.x] = bins[threadIdx.x];
}
__global__ __launch_bounds__( 256 ) void radixScatterKernel( const uint64_t* __restrict__ keyIn, const uint32_t* __restrict__ idxIn,
                                                              uint32_t n, int shift, uint32_t tiles,
                                                              const uint32_t* __restrict__ bases, uint64_t* __restrict__ keyOut,
                                                              uint32_t* __restrict__ idxOut ) {
  __shared__ uint32_t running[256], waveCount[4][256];
  const int           lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  running[threadIdx.x] = bases[size_t( threadIdx.x ) * tiles + blockIdx.x];
  const uint32_t base = blockIdx.x * kSortTile, end = min( n, base + uint32_t( kSortTile ) );
  for ( uint32_t sub = base; sub < end; sub += 256 ) {
#pragma unroll
    for ( int w = 0; w < 4; ++w ) waveCount[w][threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i     = sub + threadIdx.x;
    const bool     valid = i < end;
    const uint64_t k     = valid ? keyIn[i] : 0;
    const uint32_t d     = uint32_t( k >> shift ) & 0xFF;
    unsigned long long peers = __ballot( valid );
#pragma unroll
    for ( int bit = 0; bit < 8; ++bit ) {
      const unsigned long long m = __ballot( ( d >> bit ) & 1u );
      peers &= ( ( d >> bit ) & 1u ) ? m : ~m;
    }
    const uint32_t rankInWave = uint32_t( laneRank( peers, lane ) );
    if ( valid && rankInWave == 0 ) waveCount[wave][d] = uint32_t( __popcll( peers ) );
    __syncthreads();
    if ( valid ) {
      uint32_t at = running[d] + rankInWave;
      for ( int w = 0; w < wave; ++w ) at += waveCount[w][d];
      keyOut[at] = k;
      idxOut[at] = idxIn[i];
    }
    __syncthreads();
    running[threadIdx.x] += waveCount[0][threadIdx.x] + waveCount[1][threadIdx.x] + waveCount[2][threadIdx.x] + waveCount[3][threadIdx.x];
    __syncthreads();
  }
}
__global__ __launch_bounds__( 256 ) void runHeadKernel( const uint64_t* __restrict__ key, uint32_t n, uint32_t* __restrict__ head ) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if ( i < n ) head[i] = ( i == 0 || key[i] != key[i - 1] ) ? 1u : 0u;
}
}  // namespace

// keys / payload of `a` sorted; the result is in (keyA, idxA) or (keyB, idxB): returns which through *inA
int radixSortPairs( tmc2_ctx* ctx, uint64_t* keyA, uint32_t* idxA, uint64_t* keyB, uint32_t* idxB, uint32_t n, uint32_t bits, bool* inA ) {
  hipStream_t      s     = ctx->stream;
  const uint32_t   tiles = ( n + kSortTile - 1 ) / kSortTile;
  DevBuf<uint32_t> d_counts;
  TMC2_TRY( d_counts.alloc( size_t( 256 ) * tiles ) );
  bool fromA = true;
  for ( uint32_t shift = 0; shift < bits; shift += 8 ) {
    uint64_t* kin  = fromA ? keyA : keyB;
    uint32_t* iin  = fromA ? idxA : idxB;
    uint64_t* kout = fromA ? keyB : keyA;
    uint32_t* iout = fromA ? idxB : idxA;
    hipLaunchKernelGGL( radixCountKernel, dim3( tiles ), dim3( 256 ), 0, s, kin, n, int( shift ), tiles, d_counts.p );
    TMC2_TRY( exclusiveScanU32( ctx, d_counts.p, d_counts.p, size_t( 256 ) * tiles, nullptr ) );
    hipLaunchKernelGGL( radixScatterKernel, dim3( tiles ), dim3( 256 ), 0, s, kin, iin, n, int( shift ), tiles, d_counts.p, kout, iout );
    fromA = !fromA;
  }
  TMC2_HIP( hipGetLastError() );
  *inA = fromA;
  return TMC2_OK;
}

int markRunHeads( tmc2_ctx* ctx, const uint64_t* d_key, uint32_t n, uint32_t* d_head ) {
  if ( n ) hipLaunchKernelGGL( runHeadKernel, dim3( ( n + 255 ) / 256 ), dim3( 256 ), 0, ctx->stream, d_key, n, d_head );
  TMC2_HIP( hipGetLastError() );
  return TMC2_OK;
}

}  // namespace tmc2
